#!/usr/bin/env python3
"""Read-length figures of the training side on one GPU (ns_read_lengths; DESIGN §9, "Read lengths: the KDE inputs" — not the headline
bench): the kernel time of the fixture's records, and of a synthetic training set made by REPEATING THE FIXTURE'S CIGARs.

A synthetic record is the text of consecutive CIGARs of tests/golden/reference_read_len.json.gz, taken cyclically from a start that
differs per record, until it holds --ops ops (clips in the middle of such a text are still ops the walk sums: it stays a legal input).
599 distinct records are built and tiled to --records; reads are runs of 1, 2, 3, 1, 2, 3 ... records on one reference.  Prints one JSON
line: kernel milliseconds of every step (device events around the order sort, k_len_scan, k_len_flag, the scan and k_len_reduce), the
CIGAR bytes, GB/s over them and the fraction of the 8 TB/s the other rows of DESIGN §9 use.

    python scripts/bench_read_lengths.py [--records 1000000] [--ops 3000] [--steps 3]
"""
import argparse
import ctypes as C
import gzip
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nanosim_amd import characterize, engine as E  # noqa: E402

HBM_BYTES_PER_S = 8e12


def synthetic(cigars, n_records, n_ops):
    """(CIGAR bytes with 16 spare, offsets, ops per distinct record): len(cigars) distinct records tiled to n_records"""
    counts = [len(re.findall(r"[A-Z=]", c)) for c in cigars]
    distinct, ops = [], []
    for j in range(len(cigars)):
        parts, got, i = [], 0, (7 * j) % len(cigars)
        while got < n_ops:
            if counts[i] < 1000 and "N" not in cigars[i]:          # (not the 5 000-op record, not the introns: sums stay far below 2^32)
                parts.append(cigars[i])
                got += counts[i]
            i = (i + 1) % len(cigars)
        distinct.append("".join(parts).encode())
        ops.append(got)
    block = np.frombuffer(b"".join(distinct), dtype=np.uint8)
    lens = np.array([len(d) for d in distinct], dtype=np.uint64)
    reps = (n_records + len(distinct) - 1) // len(distinct)
    data = np.concatenate([np.tile(block, reps), np.zeros(16, dtype=np.uint8)])
    off = np.zeros(reps * len(distinct) + 1, dtype=np.uint64)
    np.cumsum(np.tile(lens, reps), out=off[1:])
    return data, off[:n_records + 1].copy(), ops


def call(eng, data, off, steps):
    n = len(off) - 1
    sizes = np.tile(np.array([1, 2, 3], dtype=np.uint64), n // 6 + 1)
    read_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    read_off = np.concatenate([read_off[read_off < n], [n]]).astype(np.uint64)
    n_reads = len(read_off) - 1
    reverse = (np.arange(n) % 2).astype(np.uint8)
    ref_id = np.zeros(n, dtype=np.uint32)
    start = ((np.arange(n, dtype=np.uint64) * 1009) % 1000000).astype(np.uint64)
    total = np.array([10 ** 9], dtype=np.uint64)
    reads, seg = np.zeros(n_reads, dtype=characterize.LEN_READ_DTYPE), np.zeros(n, dtype=np.uint64)
    out = characterize.NsLenResult()
    out.reads, out.segments = reads.ctypes.data, seg.ctypes.data
    ms, wall = [], []
    for _ in range(steps + 1):                                  # (the first call is the warm-up)
        t = time.perf_counter()
        eng._check(eng.L.ns_read_lengths(eng.ctx, data.ctypes.data, off.ctypes.data, reverse.ctypes.data, ref_id.ctypes.data, start.ctypes.data,
                                         total.ctypes.data, 1, read_off.ctypes.data, n_reads, n, characterize.LEN_GENOME, None, None, C.byref(out)))
        wall.append(time.perf_counter() - t)
        ms.append(float(out.ms_kernel))
        assert out.n_bad == 0 and int(reads["n_segments"].sum()) == out.n_segments
    return ms[1:], wall[1:], n_reads, int(out.n_segments)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--ops", type=int, default=3000)
    ap.add_argument("--steps", type=int, default=3)
    a = ap.parse_args()
    with gzip.open(os.path.join(ROOT, "tests", "golden", "reference_read_len.json.gz"), "rt") as f:
        fx = json.load(f)
    eng = E.Engine(0)
    refs, recs = [tuple(r) for r in fx["refs"]], [tuple(r) for r in fx["primary"]]
    fixture_ms = [characterize.count_read_lengths(eng, refs, recs)["ms_kernel"] for _ in range(a.steps + 1)][1:]
    data, off, ops = synthetic([r[4] for r in recs], a.records, a.ops)
    ms, wall, n_reads, n_segments = call(eng, data, off, a.steps)
    eng.close()
    nbytes = int(off[-1])
    best = min(ms)
    print(json.dumps({"metric": "ns_read_lengths kernel ms", "fixture_records": len(recs), "fixture_ms": fixture_ms, "records": a.records, "reads": n_reads,
                      "segments": n_segments, "ops_per_record": [min(ops), int(np.median(ops)), max(ops)], "cigar_bytes": nbytes, "ms_kernel": ms,
                      "wall_s": wall, "gb_per_s": nbytes / (best * 1e-3) / 1e9, "fraction_of_8_tb_s": nbytes / (best * 1e-3) / HBM_BYTES_PER_S}))


if __name__ == "__main__":
    main()
