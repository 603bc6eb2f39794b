#!/usr/bin/env python3
"""The chimeric step of the training side on one GPU (ns_chimeric_select; DESIGN §9, "Chimeric reads: the split-alignment choice" — not
the headline bench): the kernel time of the fixture's reads, and of synthetic reads with 0 .. 8 SA entries of about --ops CIGAR ops each.

A synthetic read has k = 0 .. 8 SA entries (k by turns); its pieces follow each other along the read with gaps of 0 .. 40 bases, every
fourth entry overlaps the one in front of it (a second list), references by turns.  64 distinct CIGAR bodies are drawn once and reused.
One warm-up call, then --steps timed calls.  Prints one JSON line: the median kernel milliseconds of k_chim_scan (with its visiting
order) and of k_chim_select (with its own), the CIGAR bytes and GB/s over them for each — k_chim_select does not read the text; its rate
is stated over the same bytes so that the two can be added — and the entries per second of the choice.

    python scripts/bench_chimeric_train.py [--reads 20000] [--ops 3000] [--steps 3]
"""
import argparse
import gzip
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nanosim_amd import characterize, engine as E  # noqa: E402

HBM_BYTES_PER_S = 8e12


def bodies(n_ops, rng, count=64):
    """[(text, M + I, M + D)]: `count` CIGAR bodies of n_ops ops, M runs broken by short insertions and deletions"""
    out = []
    for _ in range(count):
        m = rng.integers(1, 30, n_ops // 2 + 1)
        e = rng.integers(1, 4, n_ops // 2)
        kind = rng.integers(0, 2, n_ops // 2)
        parts = []
        for i in range(n_ops // 2):
            parts.append("%dM%d%s" % (m[i], e[i], "ID"[kind[i]]))
        parts.append("%dM" % m[-1])
        out.append(("".join(parts), int(m.sum() + e[kind == 0].sum()), int(m.sum() + e[kind == 1].sum())))
    return out


def synthetic(n_reads, n_ops, seed=1):
    """the reads of chimeric_call: [[(cigar, ref_id, ref_start, nm, reverse), ...]]"""
    rng = np.random.default_rng(seed)
    B = bodies(n_ops, rng)
    reads = []
    for r in range(n_reads):
        k = r % 9
        at, entries = int(rng.integers(0, 50)), []
        for j in range(k + 1):
            text, qlen, rlen = B[(r + 7 * j) % len(B)]
            if j and j % 4 == 0:
                at -= qlen // 2                              # overlaps the piece in front of it
            entries.append(("%dS%s" % (at, text) if at else text, (r + j) % 3, 1000 + 200000 * j + r % 1000, int(rng.integers(0, 50)), bool((r + j) % 2)))
            at += qlen + int(rng.integers(0, 41))
        order = [0] + [int(i) for i in 1 + rng.permutation(k)]   # (SA tags list the entries in no particular order)
        reads.append([entries[i] for i in order])
    return reads


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20000)
    ap.add_argument("--ops", type=int, default=3000)
    ap.add_argument("--steps", type=int, default=3)
    a = ap.parse_args()
    with gzip.open(os.path.join(ROOT, "tests", "golden", "reference_chimeric_train.json.gz"), "rt") as f:
        fx = json.load(f)
    eng = E.Engine(0)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "fixture.sam")
        with open(path, "w") as f:
            f.write(fx["sam"])
        refs, records, _, _ = characterize.chimeric_records(path)
    fixture_ms = [characterize.select_chimeric(eng, refs, records)["ms_kernel"] for _ in range(a.steps + 1)][1:]
    reads = synthetic(a.reads, a.ops)
    n_ent = sum(len(r) for r in reads)
    nbytes = sum(len(e[0]) for r in reads for e in r)
    total = [10 ** 9] * 3
    scan, select, wall, pieces, gaps = [], [], [], 0, 0
    for _ in range(a.steps + 1):                                # (the first call is the warm-up)
        t = time.perf_counter()
        out, _, _, per_read, _, _ = characterize.chimeric_call(eng, reads, total, [0, 0, 1], 2)
        wall.append(time.perf_counter() - t)
        assert out.n_bad == 0
        scan.append(float(out.ms_scan))
        select.append(float(out.ms_kernel - out.ms_scan))
        pieces, gaps = int(per_read["n_pieces"].sum()), int(out.n_gaps)
    eng.close()
    scan_ms, select_ms = float(np.median(scan[1:])), float(np.median(select[1:]))
    rate = lambda ms: nbytes / (ms * 1e-3) / 1e9
    print(json.dumps({"metric": "ns_chimeric_select kernel ms", "fixture_reads": fx["n_reads"], "fixture_ms": fixture_ms, "reads": a.reads, "entries": n_ent,
                      "ops_per_entry": a.ops + 1, "cigar_bytes": nbytes, "pieces": pieces, "gaps": gaps, "runs": a.steps, "scan_ms": scan[1:], "select_ms": select[1:],
                      "wall_s": wall[1:], "scan_ms_median": scan_ms, "select_ms_median": select_ms, "scan_gb_per_s": rate(scan_ms),
                      "select_gb_per_s": rate(select_ms), "select_entries_per_s": n_ent / (select_ms * 1e-3),
                      "scan_fraction_of_8_tb_s": nbytes / (scan_ms * 1e-3) / HBM_BYTES_PER_S}))


if __name__ == "__main__":
    main()
