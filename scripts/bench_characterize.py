#!/usr/bin/env python3
"""Training-side histogramming throughput on one GPU (not the headline bench): cs strings of N synthetic alignments (built from the event
lists of reads the engine itself generates with the hg002-like model, ~1 KB of cs per 8 kb read) through ns_cs_histograms; prints
alignments/s, the kernel's own time and its fraction of the HBM roofline (algorithmic bytes = the cs strings, read once).
    python scripts/bench_characterize.py [--alignments 200000]
--qualities: the base-quality histograms instead (ns_qual_histograms: the same cs strings plus a QUAL string per alignment, ~8.4 KB per
read): milliseconds of the two phases (the mark phase alone from a second context with NS_DEBUG_SKIP = 1 << 20, the count phase as the
difference), the end-to-end time, GB/s over cs + quality bytes — as measured and scaled to 10^6 alignments.
    python scripts/bench_characterize.py --qualities [--alignments 200000]
--homopolymers: the homopolymer-length model instead (ns_hp_histograms, min_hp_len 5): the same reads as aligned line pairs — the
reference's letters along a piece, `-` for the gaps, the events as mismatched / inserted / deleted columns —, ~8.5 KB per line; prints
alignments/s, the kernels' time (k_hp_count alone; with --records also the scan and k_hp_records) and GB/s over both lines.
--host-walk times the same walk compiled for the host (tests/hp_train_host.cpp) on one core over the same input; --dump-maf PATH writes
the first 2 000 pairs as `s` lines (what the reference's analyze_homopolymers reads).
    python scripts/bench_characterize.py --homopolymers [--records] [--host-walk] [--dump-maf PATH] [--alignments 200000]
--sam-pairs: the SAM route to that model (ns_sam_pairs_build, ns_hp_histograms_sam): the same line pairs turned into CIGAR, MD and SEQ
(2 000 distinct reads, repeated), and from there back into lines on the GPU.  Prints the kernel milliseconds of the two phases (the scan
phase from the call without line buffers, the line phase as the difference to the call with them), GB/s of lines written, the end-to-end
time of pairs_from_sam with packing, and the fused call against pairs_from_sam followed by count_homopolymers — every figure with the
values of the single steps, so that the spread shows.
    python scripts/bench_characterize.py --sam-pairs [--alignments 50000] [--steps 5]
--mixfit: the fit of the error-length mixtures (ns_mixture_fit: 512 + 9 216 + 9 216 Nelder-Mead searches, one wavefront each) on the three
histograms of the reference's fixture (7, 12 and 8 bins; tests/golden/reference_mixfit.json.gz) and on histograms of 1 000 bins: the
kernel milliseconds per type (device events around each of the three calls) of every step, the evaluations the searches made, and the
end-to-end time of fit_mixtures.
    python scripts/bench_characterize.py --mixfit [--steps 3]
--besthit: the best hit per read of a LAST MAF file (ns_maf_besthit) on a synthetic file built here: --alignments pairs of `s` lines over a
third as many read names (sizes from a small range, so that ties occur), aligned sequences of --columns bytes (200 distinct ones,
repeated), an `a score=` line and a blank line per pair.  Prints the kernel milliseconds of every step (device events from the first
kernel to the last, the host's two waits inside the call included), that per 10^6 pairs and as GB/s over the bytes of the text, and the
end-to-end time of besthit_call (the H2D copy of the text and the copies of the result included) next to the time the host needs to
read the same file into memory — the parse-and-copy side of the call.
    python scripts/bench_characterize.py --besthit [--alignments 200000] [--columns 1000] [--steps 3]
--bam: BAM input (ns_bam_to_sam, characterize.read_bam) on a synthetic file built here with the test-side writer (tests/bam_lib.py):
--alignments records of 8 kb reads (200 distinct ones, repeated) with SEQ, QUAL, a CIGAR of ~1 500 ops and NM:i, ms:i, de:f, tp:A and cs:Z
tags (the cs of the hg002-like error rates, ~2 KB).  Prints the kernel milliseconds of every step for all records in ONE call (device
events from the first kernel to the last, the host's waits and its formatting of the floats included), that per 10^5 records, the text
bytes written per second and against the 8 TB/s roofline; and, end to end, records/s of read_bam + cs_from_sam over the BAM file (BGZF
inflate, batches of 64 MB, decode, the reader's loop) next to cs_from_sam over the SAM text of the same records (bam_to_sam wrote it).
    python scripts/bench_characterize.py --bam [--alignments 20000] [--steps 3]
--calmd: MD and cs text from the reference genome (ns_calmd, characterize.with_reference) on synthetic 8 kb reads over a random genome
of 24 Mb: --alignments records (200 distinct ones, repeated; ~950 CIGAR ops each, a mismatch, an insertion or a deletion every ~11
bases) in ONE call.  Prints the kernel milliseconds of every step (device events from the first kernel to the last, the host's wait for
the sizes of the texts included), that per 10^5 records and as text bytes per second; the time of the SAME walk compiled for the host
with one lane (tests/calmd_host.cpp, -O2) on one thread over the same records, and the ratios; and, end to end, records/s of iterating
with_reference over the SAM text and over read_bam of the BAM file of the same records.
    python scripts/bench_characterize.py --calmd [--alignments 20000] [--steps 3]"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nanosim_amd import characterize, engine as E, model as M, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--alignments", type=int, default=200_000)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--qualities", action="store_true")
ap.add_argument("--homopolymers", action="store_true")
ap.add_argument("--sam-pairs", action="store_true")
ap.add_argument("--mixfit", action="store_true")
ap.add_argument("--besthit", action="store_true")
ap.add_argument("--columns", type=int, default=1000)
ap.add_argument("--bam", action="store_true")
ap.add_argument("--calmd", action="store_true")
ap.add_argument("--records", action="store_true")
ap.add_argument("--host-walk", action="store_true")
ap.add_argument("--dump-maf", default=None)
a = ap.parse_args()
SEED = 20260926
if a.mixfit:
    import gzip
    with gzip.open(os.path.join(ROOT, "tests", "golden", "reference_mixfit.json.gz"), "rt") as f:
        fx = json.load(f)
    rng = np.random.default_rng(SEED)

    def long_hist(first):
        """20 000 geometric lengths and a thin tail that reaches length 1 000 (mismatch: 1 001): 1 000 bins"""
        h = {}
        for v in np.concatenate((rng.geometric(0.02, 20000), rng.integers(1, 1001, 400), [1000])).tolist():
            h[min(v, 1000) + first] = h.get(min(v, 1000) + first, 0) + 1
        return h
    sets = {"fixture": {t: {int(k): int(v) for k, v in fx["a"]["hist"][t]} for t in ("mis", "ins", "del")},
            "1000 bins": {"mis": long_hist(1), "ins": long_hist(0), "del": long_hist(0)}}
    eng = E.Engine(0)
    res = {"metric": "error-length mixtures, kernel ms per type (ns_mixture_fit: 512 + 9216 + 9216 searches)", "steps": a.steps,
           "reference_model_fitting_wall_s": fx["a"]["model_fitting_wall_s"], "reference_cores": fx["a"]["model_fitting_cores"]}
    for name, hists in sets.items():
        characterize.fit_mixtures(eng, hists)                 # warms up
        ms, e2e = {"mis": [], "ins": [], "del": []}, []
        for _ in range(a.steps):
            t0 = time.perf_counter()
            fit = characterize.fit_mixtures(eng, hists)
            e2e.append(time.perf_counter() - t0)
            for t in ms:
                ms[t].append(fit[t]["ms_kernel"])
        evals = {}
        for t in ms:
            e = "mis" if t == "mis" else "indel"
            evals[t] = int(characterize.mixture_fit(eng, e, characterize.empirical_cdf(hists[t], e)[0], characterize.fit_starts(e))["nfev"].sum())
        res[name] = {"bins": {t: len(characterize.empirical_cdf(hists[t], "mis" if t == "mis" else "indel")[0]) for t in ms}, "kernel_ms": ms,
                     "kernel_ms_all_three(median)": float(sum(np.median(v) for v in ms.values())), "evaluations": evals,
                     "fit_mixtures_end_to_end_s": e2e, "residual": {t: fit[t]["residual"] for t in ms}, "warning": {t: fit[t]["warning"] for t in ms}}
    res["value"] = res["fixture"]["kernel_ms_all_three(median)"]
    print(json.dumps(res))
    eng.close()
    sys.exit(0)
if a.bam:
    from concurrent.futures import ThreadPoolExecutor
    from tests import bam_lib
    rng = np.random.default_rng(SEED)
    n = a.alignments if a.alignments != 200_000 else 20_000
    distinct = []
    for k in range(200):
        l_seq = int(rng.integers(7600, 8400))
        seq = "".join(rng.choice(list("ACGT"), l_seq).tolist())
        qual = rng.integers(33 + 2, 33 + 40, l_seq).astype(np.uint8).tobytes().decode()
        ops, cs, left = [], [], l_seq - 60
        while left > 0:                                           # ~ one error per 11 bases: match runs with a mismatch, an insertion or a deletion between
            m = int(min(left, rng.geometric(0.09)))
            ops.append("%dM" % (m + 1)); cs.append(":%d*ag" % m); left -= m + 1
            if left > 3 and rng.random() < 0.5:
                e = int(rng.integers(1, 4))
                if rng.random() < 0.5:
                    ops.append("%dI" % e); cs.append("+" + "acg"[:e]); left -= e
                else:
                    ops.append("%dD" % e); cs.append("-" + "tgc"[:e])
        cigar = "30S" + "".join(ops) + "30S"
        tags = (bam_lib.tag_bytes("NM", "S", 700 + k) + bam_lib.tag_bytes("ms", "i", 9000 + k) + bam_lib.tag_bytes("de", "f", 0.08 + k * 1e-4) +
                bam_lib.tag_bytes("tp", "A", "P") + bam_lib.tag_bytes("cs", "Z", "".join(cs)))
        distinct.append(bam_lib.record("read_%06d/%s" % (k, "x" * (k % 16)), 16 * (k & 1), k % 24, 1 + k * 1013, 60, cigar, -1, 0, 0, seq, qual, tags))
    refs = [("chr%d" % (i + 1), 250_000_000 - i * 1_000_000) for i in range(24)]
    header = "@HD\tVN:1.6\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs) + "@PG\tID:minimap2\tPN:minimap2\n"
    records = b"".join(distinct[i % 200] for i in range(n))
    n_ops = float(np.mean([int.from_bytes(r[16:18], "little") for r in distinct]))
    tmp = tempfile.mkdtemp(prefix="nsbam_")
    bam_path, sam_path = os.path.join(tmp, "synthetic.bam"), os.path.join(tmp, "synthetic.sam")
    inflated = bam_lib.bam_header(header, refs) + records
    with ThreadPoolExecutor(max_workers=16) as pool, open(bam_path, "wb") as f:
        for blk in pool.map(lambda i: bam_lib.bgzf_block(inflated[i:i + 65280], level=1), range(0, len(inflated), 65280)):
            f.write(blk)
        f.write(bam_lib.EOF_BLOCK)
    del inflated
    eng = E.Engine(0)
    names, off = characterize._pack([r[0] for r in refs])
    r = characterize.bam_call(eng, records, True, names, off)    # warms up
    assert int(r.n_records) == n and not r.bad_reason
    n_text, ms, call_s = int(r.n_text), [], []
    for _ in range(a.steps):
        t0 = time.perf_counter()
        r = characterize.bam_call(eng, records, True, names, off)
        call_s.append(time.perf_counter() - t0)
        ms.append(float(r.ms_kernel))
    med = float(np.median(ms))
    assert characterize.bam_to_sam(bam_path, sam_path, eng) == n and os.path.getsize(sam_path) == n_text + len(header)
    from_bam, from_sam = [], []
    for _ in range(a.steps):
        t0 = time.perf_counter()
        cs_bam = characterize.cs_from_sam(characterize.read_bam(bam_path, eng))
        from_bam.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        cs_sam = characterize.cs_from_sam(sam_path)
        from_sam.append(time.perf_counter() - t0)
        assert cs_bam == cs_sam and len(cs_sam) == n
    print(json.dumps({"metric": "BAM records to SAM text, kernel ms per 10^5 records of 8 kb reads with cs tags (ns_bam_to_sam)", "value": med * 1e5 / n,
                      "records": n, "record_bytes": len(records), "text_bytes": n_text, "cigar_ops_per_record": n_ops, "steps": a.steps, "kernel_ms": ms,
                      "text_gb_per_s": n_text / (med * 1e-3) / 1e9, "text_frac_of_hbm_8tbs": n_text / (med * 1e-3) / 1e9 / 8000.0,
                      "moved_gb_per_s(records read + text written)": (len(records) + n_text) / (med * 1e-3) / 1e9,
                      "bam_call_end_to_end_s": call_s, "bam_file_bytes": os.path.getsize(bam_path),
                      "read_bam+cs_from_sam_s": from_bam, "cs_from_sam(sam text)_s": from_sam,
                      "records_per_s(read_bam + cs_from_sam)": n / float(np.median(from_bam)),
                      "records_per_s(cs_from_sam over SAM text)": n / float(np.median(from_sam))}))
    eng.close()
    os.remove(bam_path)
    os.remove(sam_path)
    os.rmdir(tmp)
    sys.exit(0)
if a.calmd:
    import subprocess
    import types
    from concurrent.futures import ThreadPoolExecutor
    from tests import bam_lib
    rng = np.random.default_rng(SEED)
    n = a.alignments if a.alignments != 200_000 else 20_000
    n_chrom, chrom_len = 24, 1_000_000
    ref = M.make_reference(["chr%d" % (i + 1) for i in range(n_chrom)],
                           [np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, chrom_len)] for _ in range(n_chrom)])
    distinct = []                                                 # (cigar, seq, chrom, pos)
    for k in range(200):
        ci, start = k % n_chrom, int(rng.integers(0, chrom_len - 10_000))
        chrom = ref.chrom(ci).tobytes().decode()
        want, r, ops, seq = int(rng.integers(7600, 8400)), start, [], ["A" * 30]
        while len(ops) < 4 or sum(len(s) for s in seq) < want:   # ~ one error per 11 bases: match runs with a mismatch, an insertion or a deletion between
            m = int(rng.geometric(0.09))
            seq.append(chrom[r:r + m] + "ACGT"[("ACGT".index(chrom[r + m]) + 1) % 4]); ops.append("%dM" % (m + 1)); r += m + 1
            if rng.random() < 0.5:
                e = int(rng.integers(1, 4))
                if rng.random() < 0.5:
                    ops.append("%dI" % e); seq.append("acg"[:e])
                else:
                    ops.append("%dD" % e); r += e
        seq.append(chrom[r:r + 5] + "C" * 30); ops.append("5M")
        distinct.append(("30S" + "".join(ops) + "30S", "".join(seq), ci, start + 1))
    recs = [distinct[i % 200] for i in range(n)]
    cigars, seqs, chroms, poss = [x[0] for x in recs], [x[1] for x in recs], [x[2] for x in recs], [x[3] for x in recs]
    n_ops = float(np.mean([x[0].count("M") + x[0].count("I") + x[0].count("D") + 2 for x in distinct]))
    seq_bytes = sum(len(s) for s in seqs)
    eng = E.Engine(0)
    eng.set_reference(ref)
    r = characterize.cs_md_call(eng, cigars, seqs, chroms, poss)    # warms up
    n_text, ms, call_s = len(r["md"]) + len(r["cs"]), [], []
    for _ in range(a.steps):
        t0 = time.perf_counter()
        r = characterize.cs_md_call(eng, cigars, seqs, chroms, poss)
        call_s.append(time.perf_counter() - t0)
        ms.append(r["ms_kernel"])
    med = float(np.median(ms))
    # the same walk, compiled for the host with one lane, on one thread over the same records
    tmp = tempfile.mkdtemp(prefix="nscalmd_")
    so = os.path.join(tmp, "libcalmd_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tests", "calmd_host.cpp")])
    HL = C.CDLL(so)
    HL.calmd_host.restype = C.c_int
    HL.calmd_host.argtypes = [C.c_void_p] + [C.c_void_p] * 6 + [C.c_uint32, C.c_void_p]
    HL.calmd_host_set_reference.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32]
    assert HL.calmd_host_set_reference(ref.bases.ctypes.data, len(ref.bases), ref.chrom_off.ctypes.data, len(ref.names)) == 0

    def host_check(rc):
        assert rc == 0, rc
    host = types.SimpleNamespace(ctx=None, _check=host_check, L=types.SimpleNamespace(ns_calmd=HL.calmd_host))
    host_ms = []
    for _ in range(a.steps):
        h = characterize.cs_md_call(host, cigars, seqs, chroms, poss)
        host_ms.append(h["ms_kernel"])
    assert h["md"] == r["md"] and h["cs"] == r["cs"]
    host_med = float(np.median(host_ms))
    # end to end: with_reference over SAM text and over the BAM file of the same records
    names = ref.names
    header = "@HD\tVN:1.6\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % (nm, chrom_len) for nm in names) + "@PG\tID:minimap2\tPN:minimap2\n"
    quals = ["".join(chr(33 + 2 + (i * 7 + k) % 38) for i in range(len(x[1]))) for k, x in enumerate(distinct)]
    sam_path, bam_path = os.path.join(tmp, "synthetic.sam"), os.path.join(tmp, "synthetic.bam")
    with open(sam_path, "w") as f:
        f.write(header)
        for i in range(n):
            c, s, ci, p = distinct[i % 200]
            f.write("read_%06d\t%d\t%s\t%d\t60\t%s\t*\t0\t0\t%s\t%s\tNM:i:700\n" % (i, 16 * (i & 1), names[ci], p, c, s, quals[i % 200]))
    packed = [bam_lib.record("read_%06d" % k, 16 * (k & 1), x[2], x[3], 60, x[0], -1, 0, 0, x[1].upper(), quals[k], bam_lib.tag_bytes("NM", "S", 700))
              for k, x in enumerate(distinct)]
    inflated = bam_lib.bam_header(header, [(nm, chrom_len) for nm in names]) + b"".join(packed[i % 200] for i in range(n))
    with ThreadPoolExecutor(max_workers=16) as pool, open(bam_path, "wb") as f:
        for blk in pool.map(lambda i: bam_lib.bgzf_block(inflated[i:i + 65280], level=1), range(0, len(inflated), 65280)):
            f.write(blk)
        f.write(bam_lib.EOF_BLOCK)
    del inflated
    over_sam, over_bam = [], []
    for _ in range(a.steps):
        t0 = time.perf_counter()
        tagged = characterize.with_reference(sam_path, ref, eng)
        got = sum(1 for line in tagged if line[0] != "@")
        over_sam.append(time.perf_counter() - t0)
        assert got == n == tagged.n_tagged
        t0 = time.perf_counter()
        tagged = characterize.with_reference(characterize.read_bam(bam_path, eng), ref, eng)
        got = sum(1 for line in tagged if line[0] != "@")
        over_bam.append(time.perf_counter() - t0)
        assert got == n == tagged.n_tagged
    print(json.dumps({"metric": "MD and cs text from the reference, kernel ms per 10^5 records of 8 kb reads (ns_calmd)", "value": med * 1e5 / n,
                      "records": n, "seq_bytes": seq_bytes, "text_bytes": n_text, "cigar_ops_per_record": n_ops, "steps": a.steps, "kernel_ms": ms,
                      "text_gb_per_s": n_text / (med * 1e-3) / 1e9, "bases_gb_per_s(SEQ + reference read, both walks)": 4.0 * seq_bytes / (med * 1e-3) / 1e9,
                      "cs_md_call_end_to_end_s": call_s, "host_walk_one_thread_ms": host_ms, "host_walk_ms_per_1e5_records": host_med * 1e5 / n,
                      "host_one_thread_over_gpu_kernel": host_med / med, "host_sixteen_threads_worth_over_gpu_kernel": host_med / 16.0 / med,
                      "host_one_thread_over_gpu_call": host_med * 1e-3 / float(np.median(call_s)),
                      "with_reference_over_sam_s": over_sam, "with_reference_over_bam_s": over_bam,
                      "records_per_s(with_reference over SAM text)": n / float(np.median(over_sam)),
                      "records_per_s(with_reference over read_bam)": n / float(np.median(over_bam))}))
    eng.close()
    for p in (so, sam_path, bam_path):
        os.remove(p)
    os.rmdir(tmp)
    sys.exit(0)
if a.besthit:
    rng = np.random.default_rng(SEED)
    seqs = ["".join(rng.choice(list("ACGT-"), a.columns, p=[0.24, 0.24, 0.24, 0.24, 0.04]).tolist()) for _ in range(200)]
    n_names = max(1, a.alignments // 3)
    name_id, size = rng.integers(0, n_names, a.alignments).tolist(), rng.integers(a.columns // 2, a.columns // 2 + 50, a.alignments).tolist()
    parts = ["# LAST version 1256\n"]
    for i in range(a.alignments):
        sq = seqs[i % 200]
        parts.append("a score=%d\ns chr%d %9d %d + 248956422 %s\ns read_%08x %5d %d %s %d %s\n\n"
                     % (size[i] * 6, i % 24, i * 13, a.columns, sq, name_id[i], i % 50, size[i], "+-"[i & 1], size[i] + 120, sq))
    tmp = tempfile.mkdtemp(prefix="nsbest_")
    path = os.path.join(tmp, "synthetic.maf")
    with open(path, "w") as f:
        f.write("".join(parts))
    del parts
    nbytes = os.path.getsize(path)
    best = {}
    for i in range(a.alignments):                             # the choice restated (G:14-39): how many pairs have to be kept
        if best.get(name_id[i], -1) < size[i]:
            best[name_id[i]] = size[i]
    eng = E.Engine(0)
    host_read_s = []
    for _ in range(a.steps + 1):
        t0 = time.perf_counter()
        text = np.fromfile(path, dtype=np.uint8)
        host_read_s.append(time.perf_counter() - t0)
    r = characterize.besthit_call(eng, text)                  # warms up
    assert int(r["raw"].n_pairs) == a.alignments and int(r["raw"].n_kept) == len(best) and r["raw"].first_bad_line == r["raw"].n_lines
    ms, e2e = [], []
    for _ in range(a.steps):
        t0 = time.perf_counter()
        r = characterize.besthit_call(eng, text)
        e2e.append(time.perf_counter() - t0)
        ms.append(float(r["raw"].ms_kernel))
    med = float(np.median(ms))
    print(json.dumps({"metric": "best hit per read of a MAF file, kernel ms per 10^6 pairs (ns_maf_besthit)", "value": med * 1e6 / a.alignments,
                      "pairs": a.alignments, "names": len(best), "columns": a.columns, "text_bytes": nbytes, "steps": a.steps, "kernel_ms": ms,
                      "kernel_gb_per_s(text bytes)": nbytes / (med * 1e-3) / 1e9, "kernel_frac_of_hbm_8tbs": nbytes / (med * 1e-3) / 1e9 / 8000.0,
                      "besthit_call_end_to_end_s": e2e, "host_read_of_the_file_s": host_read_s[1:],
                      "end_to_end_gb_per_s": nbytes / float(np.median(e2e)) / 1e9}))
    eng.close()
    os.remove(path)
    os.rmdir(tmp)
    sys.exit(0)
tmp = tempfile.mkdtemp(prefix="nschar_")
prefix = os.path.join(tmp, "hg002_like")
synth.write_model(prefix, synth.SynthModelSpec(n_train=200_000, seed=SEED), write_pkl=False)
mdl = M.load_model(prefix)
seq = synth.synth_sequence(synth.ECOLI_LEN, SEED, n_frac=0.0005, iupac_frac=0.0002, lower_frac=0.02, hp_boost=0.005)
ref = M.Reference(["ecoli-like"], seq, np.array([0, len(seq)], dtype=np.uint64), np.array([1], dtype=np.uint8))
eng = E.Engine(0)
eng.set_reference(ref)
eng.load_model(mdl)
n_src = min(a.alignments, 2_000 if a.sam_pairs else 20_000)   # cs strings of 20 000 reads, repeated up to the requested number
b = eng.generate(E.make_params(seed=SEED, first_read=0, n_reads=n_src, max_len=ref.max_chrom, emit_records=False))
pieces, events = b.pieces(), b.events()
rng = np.random.default_rng(SEED)
letters = np.frombuffer(b"acgt", dtype=np.uint8)
if a.homopolymers or a.sam_pairs:
    # the two lines of an alignment: the reference's letters from a random place of the genome (its homopolymer runs included), the
    # events of the piece as columns
    pairs = []
    dash = ord("-")
    other = np.full(256, ord("A"), dtype=np.uint8)            # the letter a mismatch column shows: another one than the reference's
    other[np.frombuffer(b"ACGTacgt", dtype=np.uint8)] = np.frombuffer(b"CGTACGTA", dtype=np.uint8)
    for pc in pieces:
        ev = events[int(pc["ev_off"]):int(pc["ev_off"]) + int(pc["n_ev"])]
        n = int(pc["ref_len"])
        at = int(rng.integers(0, len(seq) - n - 1))
        r = seq[at:at + n].copy()
        q = r.copy()
        ins_at, ins_n = [], []
        for e in ev:
            epos, ln, ty = int(e["pos"]), int(e["info"]) & 0xfff, (int(e["info"]) >> 12) & 3
            if ty == 0:
                q[epos:epos + ln] = other[r[epos:epos + ln]]
            elif ty == 1:
                ins_at.append(epos); ins_n.append(ln)
            else:
                q[epos:epos + ln] = dash
        if ins_at:
            where = np.repeat(np.minimum(ins_at, n), ins_n)
            r, q = np.insert(r, where, dash), np.insert(q, where, letters[rng.integers(0, 4, len(where))] - 32)
        pairs.append((r.tobytes(), q.tobytes()))
    if a.sam_pairs:
        def sam_of_columns(r, q):
            """(CIGAR, MD, SEQ) of an aligned line pair (uint8 arrays)"""
            op = np.where(r == dash, 1, np.where(q == dash, 2, 0))                     # M, I, D
            starts = np.concatenate(([0], np.flatnonzero(np.diff(op)) + 1))
            lens = np.diff(np.concatenate((starts, [len(op)])))
            cigar = "".join("%d%s" % (n, "MID"[o]) for n, o in zip(lens.tolist(), op[starts].tolist()))
            keep = op != 1
            rr, dd = r[keep], op[keep] == 2
            md, prev, in_del = [], -1, False
            for i in np.flatnonzero(dd | (rr != q[keep])).tolist():
                if dd[i] and in_del and i == prev + 1:
                    md.append(chr(rr[i]))                                               # (a `^` run goes on over an insertion)
                else:
                    md.append("%d%s%s" % (i - prev - 1, "^" if dd[i] else "", chr(rr[i])))
                in_del, prev = bool(dd[i]), i
            md.append(str(len(rr) - prev - 1))
            return cigar, "".join(md), q[q != dash].tobytes().decode()
        src = [("read%d" % i, 0, "ref", 1) + sam_of_columns(np.frombuffer(r, dtype=np.uint8), np.frombuffer(q, dtype=np.uint8)) for i, (r, q) in enumerate(pairs)]
        recs = (src * (a.alignments // len(src) + 1))[:a.alignments]
        tuples = [("ref", 0, r.decode(), q.decode()) for r, q in (pairs * (a.alignments // len(pairs) + 1))[:a.alignments]]
        in_bytes = sum(len(x[4]) + len(x[5]) + len(x[6]) for x in recs)
        packed = characterize.pairs_from_sam(eng, recs)                                # warms up; the result is checked once
        n_lines = int(packed.off[-1])
        assert all(packed[i] == tuples[i] for i in range(0, len(recs), max(1, len(recs) // 50)))
        args, keep_alive = characterize._pack_sam(recs)

        def build_ms(lines):
            p, bufs = characterize._sam_out(recs, keep_alive, lines)
            eng._check(eng.L.ns_sam_pairs_build(eng.ctx, *args, len(recs), C.byref(p)))
            return float(p.ms_kernel)
        build_ms(True)
        ms_scan = [build_ms(False) for _ in range(a.steps)]
        ms_both = [build_ms(True) for _ in range(a.steps)]
        e2e = []
        for _ in range(a.steps):
            t0 = time.perf_counter()
            packed = characterize.pairs_from_sam(eng, recs)
            e2e.append(time.perf_counter() - t0)
        t = characterize.count_homopolymers_sam(eng, recs, 5)                          # sizes the table, warms up
        caps = dict(cap_ref=max(64, 1 << int(t["table"].shape[1] - 1).bit_length()), cap_read=max(64, 1 << int(t["table"].shape[2] - 1).bit_length()))
        fused_s, fused_ms, fused_pairs_ms, two_s, two_ms = [], [], [], [], []
        for _ in range(a.steps):
            t0 = time.perf_counter()
            f = characterize.count_homopolymers_sam(eng, recs, 5, **caps)
            fused_s.append(time.perf_counter() - t0)
            fused_ms.append(f["ms_kernel"]); fused_pairs_ms.append(f["ms_kernel_pairs"])
            t0 = time.perf_counter()
            pk = characterize.pairs_from_sam(eng, recs)
            g = characterize.count_homopolymers(eng, pk, 5, **caps)
            two_s.append(time.perf_counter() - t0)
            two_ms.append(pk.ms_kernel + g["ms_kernel"])
            assert np.array_equal(f["table"], g["table"]) and np.array_equal(f["columns"], g["columns"])
        med = lambda v: float(np.median(v))
        ms_lines = med(ms_both) - med(ms_scan)
        print(json.dumps({"metric": "SAM records to aligned line pairs, alignments/s (pairs_from_sam incl. packing + H2D + D2H)", "value": a.alignments / med(e2e),
                          "alignments": a.alignments, "steps": a.steps, "input_bytes(cigar+md+seq)": in_bytes, "line_bytes(both lines)": 2 * n_lines,
                          "line_bytes_per_alignment": 2 * n_lines / a.alignments,
                          "scan_ms(k_sam_scan + scan)": ms_scan, "both_phases_ms": ms_both, "lines_ms(k_sam_lines, difference of medians)": ms_lines,
                          "lines_gb_per_s(bytes written)": 2 * n_lines / (ms_lines * 1e-3) / 1e9 if ms_lines > 0 else None,
                          "both_phases_gb_per_s(read + written)": (in_bytes + 2 * n_lines) / (med(ms_both) * 1e-3) / 1e9,
                          "pairs_from_sam_end_to_end_s": e2e,
                          "fused_end_to_end_s": fused_s, "fused_kernels_ms": fused_ms, "fused_kernels_ms_conversion_part": fused_pairs_ms,
                          "pairs_then_count_end_to_end_s": two_s, "pairs_then_count_kernels_ms": two_ms, "homopolymers": t["n_hp"]}))
        eng.close()
        sys.exit(0)
    pairs = (pairs * (a.alignments // len(pairs) + 1))[:a.alignments]
    nbytes = 2 * sum(len(x[0]) for x in pairs)
    if a.dump_maf:
        with open(a.dump_maf, "w") as f:
            for r, q in pairs[:2000]:
                f.write("s ref 0 %d + %d %s\ns read 0 %d + %d %s\n" % (len(r) - r.count(b"-"), len(seq), r.decode(), len(q) - q.count(b"-"),
                                                                       len(q), q.decode()))
    t = characterize.count_homopolymers(eng, pairs, 5, records=a.records)          # sizes the table and the record buffer, warms up
    caps = dict(cap_ref=max(64, 1 << int(t["table"].shape[1] - 1).bit_length()), cap_read=max(64, 1 << int(t["table"].shape[2] - 1).bit_length()),
                cap_records=max(t["n_hp"], 1))
    t0 = time.perf_counter()
    ms = [characterize.count_homopolymers(eng, pairs, 5, records=a.records, **caps)["ms_kernel"] for _ in range(a.steps)]
    dt = (time.perf_counter() - t0) / a.steps
    res = {"metric": "homopolymer-length model, alignments/s (ns_hp_histograms incl. packing + H2D)", "value": a.alignments / dt,
           "alignments": a.alignments, "line_bytes": nbytes, "bytes_per_alignment": nbytes / a.alignments, "homopolymers": t["n_hp"],
           "records": bool(a.records), "kernel_ms": float(np.mean(ms)), "kernel_alignments_per_s": a.alignments / (float(np.mean(ms)) * 1e-3),
           "kernel_gb_per_s": nbytes / (float(np.mean(ms)) * 1e-3) / 1e9, "end_to_end_s": dt,
           "max_ref_len": int(t["table"].shape[1] - 1), "max_read_len": int(t["table"].shape[2] - 1)}
    if a.host_walk:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from test_hp_train import build_host_walk
        host = build_host_walk()
        th = characterize.count_homopolymers(host, pairs, 5, records=a.records, **caps)
        assert np.array_equal(th["table"], t["table"]) and np.array_equal(th["columns"], t["columns"])
        # the call alone (no packing): the shim is handed the packed buffers
        rb, qb = b"".join(x[0] for x in pairs), b"".join(x[1] for x in pairs)
        off = np.cumsum([0] + [len(x[0]) for x in pairs]).astype(np.uint64)
        h = characterize.NsHpHist()
        tab = np.zeros((2, caps["cap_ref"], caps["cap_read"]), dtype=np.uint64)
        h.cap_ref, h.cap_read, h.table = caps["cap_ref"], caps["cap_read"], tab.ctypes.data
        t0 = time.perf_counter()
        host.L.ns_hp_histograms(None, rb, qb, len(rb), off.ctypes.data, len(pairs), 5, C.byref(h))
        res["host_walk_one_core_s"] = time.perf_counter() - t0
        res["host_walk_alignments_per_s"] = a.alignments / res["host_walk_one_core_s"]
    print(json.dumps(res))
    eng.close()
    sys.exit(0)
cs, cover = [], []
for pc in pieces:
    ev = events[int(pc["ev_off"]):int(pc["ev_off"]) + int(pc["n_ev"])]
    s, pos, qn = [], 0, 0
    for e in ev:
        epos, ln, ty = int(e["pos"]), int(e["info"]) & 0xfff, (int(e["info"]) >> 12) & 3
        if epos > pos:
            s.append(":%d" % (epos - pos)); qn += epos - pos; pos = epos
        if ty == 0:
            s.append("*ac" * ln); pos += ln; qn += ln
        elif ty == 1:
            s.append("+" + "a" * ln); qn += ln
        else:
            s.append("-" + "a" * ln); pos += ln
    if int(pc["ref_len"]) > pos:
        s.append(":%d" % (int(pc["ref_len"]) - pos)); qn += int(pc["ref_len"]) - pos
    cs.append("".join(s)); cover.append(qn)
if a.qualities:
    # a QUAL string per alignment: a head and a tail clip of 0-40 bases around the bases the cs string covers, log-normal values
    clips = rng.integers(0, 41, (len(cs), 2))
    pool = (np.clip(np.rint(np.exp(rng.normal(3.0, 0.4, 1 << 24))), 1, 93).astype(np.uint8) + 33).tobytes()
    src = []
    for c, n, (hd, tl) in zip(cs, cover, clips):
        at = int(rng.integers(0, len(pool) - (n + 81)))
        src.append((c, pool[at:at + int(hd) + n + int(tl)], int(hd), int(tl)))
    aligned = (src * (a.alignments // len(src) + 1))[:a.alignments]
    nbytes = sum(len(x[0]) + len(x[1]) for x in aligned)
    characterize.count_qualities(eng, aligned)             # warms up
    t0 = time.perf_counter()
    ms = [characterize.count_qualities(eng, aligned)["ms_kernel"] for _ in range(a.steps)]
    dt = (time.perf_counter() - t0) / a.steps
    eng.close()
    os.environ["NS_DEBUG_SKIP"] = str(1 << 20)             # (read when a context is created) the count phase is left out: counts are not used
    eng = E.Engine(0)
    characterize._qual_call(eng, [x + (0,) for x in aligned])       # warms up
    ms_mark = [characterize._qual_call(eng, [x + (0,) for x in aligned]).ms_kernel for _ in range(a.steps)]
    eng.close()
    per_m = 1e6 / a.alignments
    both, mark = float(np.mean(ms)), float(np.mean(ms_mark))
    qbytes = sum(len(x[1]) for x in aligned)
    print(json.dumps({"metric": "base-quality histograms, alignments/s (ns_qual_histograms incl. packing + H2D)", "value": a.alignments / dt,
                      "alignments": a.alignments, "cs_plus_qual_bytes": nbytes, "qual_bytes_per_alignment": qbytes / a.alignments,
                      "kernels_ms": both, "mark_ms(memset+sort+k_qual_mark)": mark, "count_ms(k_qual_count, by difference)": both - mark,
                      "end_to_end_s": dt, "kernels_gb_per_s": nbytes / (both * 1e-3) / 1e9,
                      "count_gb_per_s(qual bytes + marks)": qbytes * 1.25 / ((both - mark) * 1e-3) / 1e9,
                      "count_frac_of_hbm_8tbs": qbytes * 1.25 / ((both - mark) * 1e-3) / 1e9 / 8000.0,
                      "per_1e6_alignments": {"kernels_ms": both * per_m, "mark_ms": mark * per_m, "count_ms": (both - mark) * per_m, "end_to_end_s": dt * per_m}}))
    sys.exit(0)
cs = (cs * (a.alignments // len(cs) + 1))[:a.alignments]
nbytes = sum(len(x) for x in cs)
t = characterize.count(eng, cs)                          # sizes the match matrix, warms up
t0 = time.perf_counter()
ms = []
for _ in range(a.steps):
    ms.append(characterize.count(eng, cs, cap=t["match_list"].shape[0])["ms_kernel"])
dt = (time.perf_counter() - t0) / a.steps
print(json.dumps({"metric": "training-side histogramming, alignments/s (ns_cs_histograms incl. packing + H2D)", "value": a.alignments / dt,
                  "alignments": a.alignments, "cs_bytes": nbytes, "cs_bytes_per_alignment": nbytes / a.alignments,
                  "kernel_ms": float(np.mean(ms)), "kernel_gb_per_s": nbytes / (float(np.mean(ms)) * 1e-3) / 1e9,
                  "kernel_frac_of_hbm_8tbs": nbytes / (float(np.mean(ms)) * 1e-3) / 1e9 / 8000.0, "max_match": t["max_match"]}))
eng.close()
