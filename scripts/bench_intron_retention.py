#!/usr/bin/env python3
"""The intron-retention step of the training side on one GPU (ns_ir_train; DESIGN §9, "Intron retention: the Markov counts" — not part of
bench.py).  Synthetic input built here from a seed, no file input: --trx transcripts of 10 introns each on 24 chromosomes, --reads reads
(10^6) that follow their transcript over all of its introns — an exon, then the intron spliced out (N) or, one time in seven, read
through — about 20 CIGAR ops each; 2^14 distinct reads, repeated.

Prints one JSON line: the kernel time (ms_kernel: events around the visiting order and k_ir_walk) and the time of the whole call with
the packing of the CIGAR texts in front of it (a host clock around characterize.ir_train_call, which ends in a synchronise), each as
the median of --repeat calls after one warm-up call; the bytes the kernel has to read and write (CIGAR bytes, 16 + 12 bytes of offsets
and ids per read, the row words written and read back, a state byte) and that over the kernel time.
--reference N times the reference's own loop (src/model_intron_retention.py:104-176, restated with a list of intervals per chromosome
standing in for HTSeq's GenomicArrayOfSets — a STAND-IN figure, not HTSeq's) over the first N reads on the CPU this runs on, and scales
it to --reads (--reference-only: without a GPU).

    python scripts/bench_intron_retention.py [--reads 1000000] [--trx 20000] [--repeat 5] [--reference 10000] [--reference-only]
"""
import argparse
import bisect
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nanosim_amd import characterize, engine      # noqa: E402

N_CHROM, N_INTRONS, N_DISTINCT = 24, 10, 1 << 14


def annotation(n_trx: int, seed: int) -> dict:
    """ir_introns' dict: transcript -> [(chrom, start, end)], 10 introns of 80 .. 5 000 bases between exons of 60 .. 400; the transcripts
    of a chromosome lie one behind the other"""
    rng = np.random.default_rng(seed)
    out, cursor = {}, [1000] * N_CHROM
    for t in range(n_trx):
        chrom = "c%d" % (t % N_CHROM)
        pos = cursor[t % N_CHROM] + int(rng.integers(500, 20000))
        rows = []
        for ln, ex in zip(rng.integers(80, 5000, N_INTRONS).tolist(), rng.integers(60, 400, N_INTRONS).tolist()):
            pos += ex
            rows.append((chrom, pos, pos + ln))
            pos += ln
        cursor[t % N_CHROM] = pos + 500
        out["T%d" % t] = rows
    return out


def reads_of(introns: dict, tables: dict, n_reads: int, seed: int):
    """(cigars, start, chrom id, trx id) of n_reads reads: N_DISTINCT distinct ones, repeated in a shuffled order"""
    rng = np.random.default_rng(seed)
    names = list(introns)
    cigars, start, chrom, trx = [], [], [], []
    for _ in range(min(N_DISTINCT, n_reads)):
        tid = names[int(rng.integers(0, len(names)))]
        rows = introns[tid]
        pos = rows[0][1] - int(rng.integers(20, 60))
        start.append(pos)
        ops = []
        for (_, s, e), keep in zip(rows, (rng.random(len(rows)) < 1 / 7).tolist()):
            ops.append("%dM" % (s - pos))
            ops.append("%d%s" % (e - s, "M" if keep else "N"))
            pos = e
        cigars.append("".join(ops) + "%dM" % int(rng.integers(20, 60)))
        chrom.append(tables["chrom_id"][rows[0][0]])
        trx.append(tables["trx_id"][tid])
    pick = rng.integers(0, len(cigars), n_reads)
    return ([cigars[i] for i in pick.tolist()], np.array(start, dtype=np.uint32)[pick], np.array(chrom, dtype=np.uint32)[pick],
            np.array(trx, dtype=np.uint32)[pick])


def reference_seconds(introns: dict, cigars, start, chrom_names, trx_names):
    """the loop of M:104-176 as the reference writes it, over these reads; features[iv].steps() is a bisect into one sorted list of
    (start, end, transcript) per chromosome (the synthetic transcripts do not overlap: a step is an intron or a gap) — the stand-in for HTSeq;
    -> (seconds, the six counts)"""
    per_chrom = {}
    for tid, rows in introns.items():
        for c, s, e in rows:
            per_chrom.setdefault(c, []).append((s, e, tid))
    for v in per_chrom.values():
        v.sort()
    starts = {c: [x[0] for x in v] for c, v in per_chrom.items()}
    info = {tid: [(s, e, e - s) for _, s, e in rows] for tid, rows in introns.items()}

    def steps(c, a, b):
        v, st = per_chrom.get(c, []), starts.get(c, [])
        k = max(bisect.bisect_right(st, a) - 1, 0)
        pos = a
        while pos < b:
            while k < len(v) and v[k][1] <= pos:
                k += 1
            if k < len(v) and v[k][0] <= pos:
                e = min(v[k][1], b)
                yield pos, e, {v[k][2]}
            else:
                e = min(v[k][0], b) if k < len(v) else b
                yield pos, e, set()
            pos = e
    first = {False: 0, True: 0}
    states = {(False, False): 0, (False, True): 0, (True, False): 0, (True, True): 0}
    t0 = time.perf_counter()
    for cg, st, c, trx in zip(cigars, start, chrom_names, trx_names):
        blocks, pos, num = [], st, 0
        for ch in cg:
            if ch.isdigit():
                num = num * 10 + ord(ch) - 48
                continue
            if ch in "M=X":
                blocks.append((pos, pos + num))
            if ch in "M=XDN":
                pos += num
            num = 0
        positions, plist, ir_info, length_ir = [], [], False, 0
        for a, b in blocks:
            for s, e, fs in steps(c, a, b):
                if fs.intersection(set([trx])):
                    length_ir += e - s
                    plist.append(s)
                    plist.append(e)
                elif length_ir != 0:
                    for intron in info[trx]:
                        if length_ir == intron[2]:
                            positions.append(min(plist))
                            positions.append(max(plist))
                            ir_info = True
                    length_ir = 0
                    plist = []
        rows = info[trx]
        if not ir_info:
            first[False] += 1
            states[(False, False)] += len(rows) - 1
        else:
            prev = any(rows[0][0] <= p <= rows[0][1] for p in positions)
            first[prev] += 1
            for i in range(1, len(rows)):
                cur = any(rows[i][0] <= p <= rows[i][1] for p in positions)
                states[(prev, cur)] += 1
                prev = cur
    return time.perf_counter() - t0, [first[False], first[True]] + [states[k] for k in ((False, False), (False, True), (True, False), (True, True))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--trx", type=int, default=20000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--reference", type=int, default=0)
    ap.add_argument("--reference-only", action="store_true")
    a = ap.parse_args()
    introns = annotation(a.trx, 11)
    tables = characterize.ir_tables(introns)
    cigars, start, chrom, trx = reads_of(introns, tables, a.reads, 12)
    n_ops = sum(1 for c in cigars[0] if not c.isdigit())
    cigar_bytes = sum(len(c) for c in cigars)
    row_words = a.reads * ((N_INTRONS + 31) // 32)
    traffic = cigar_bytes + a.reads * (16 + 12 + 1) + 2 * 4 * row_words
    out = {"metric": "ns_ir_train", "reads": a.reads, "transcripts": a.trx, "introns": int(tables["intr_off"][-1]), "cigar_ops_per_read": n_ops,
           "cigar_bytes": cigar_bytes, "kernel_bytes": traffic, "repeat": a.repeat}
    if a.reference or a.reference_only:
        n = min(max(a.reference, 1), a.reads)
        chrom_names, trx_names = list(tables["chrom_id"]), list(tables["trx_id"])
        secs, ref_counts = reference_seconds(introns, cigars[:n], start[:n].tolist(), [chrom_names[i] for i in chrom[:n].tolist()],
                                             [trx_names[i] for i in trx[:n].tolist()])
        out.update({"reference_standin_reads": n, "reference_standin_cpu_s": secs, "reference_standin_cpu_s_scaled_to_reads": secs * a.reads / n})
    if not a.reference_only:
        eng = engine.Engine(0)
        try:
            characterize.ir_train_call(eng, tables, cigars, start, chrom, trx)               # warm-up
            ms_kernel, ms_call = [], []
            for _ in range(a.repeat):
                t0 = time.perf_counter()
                res, state, bits = characterize.ir_train_call(eng, tables, cigars, start, chrom, trx)
                ms_call.append((time.perf_counter() - t0) * 1e3)
                ms_kernel.append(float(res.ms_kernel))
            counts = [int(v) for v in res.first] + [int(v) for v in res.states]
            if a.reference:                                                                  # the same counts on the reads both walked
                res_n = characterize.ir_train_call(eng, tables, cigars[:n], start[:n], chrom[:n], trx[:n])[0]
                assert [int(v) for v in res_n.first] + [int(v) for v in res_n.states] == ref_counts, "the GPU and the restated loop disagree"
            ms = statistics.median(ms_kernel)
            out.update({"ms_kernel": ms, "ms_kernel_min": min(ms_kernel), "ms_kernel_max": max(ms_kernel), "ms_call_with_packing": statistics.median(ms_call),
                        "kernel_GB_per_s": traffic / ms / 1e6, "share_of_8_TB_per_s": traffic / ms / 1e6 / 8000.0, "counts": counts, "n_bad": int(res.n_bad),
                        "retained_introns": int(bits.sum())})
        finally:
            eng.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
