#!/usr/bin/env python3
"""The quantification EM of the training side on one GPU (ns_em_quantify; DESIGN §9, "Quantification: the EM in the reference's order" —
not part of bench.py).  Synthetic problems built here, no file input:

  trans   2*10^5 transcripts, 2*10^6 reads, 30 % of them multi-mapping with 2 - 4 candidates;
  meta    10 species, 10^6 reads, 30 % of them multi-mapping with 2 - 3 candidates.

Prints one JSON line per problem: n_iter, the time of the whole call's loop (ms_kernel: events around all iterations, the reads of the
stop flag included) as the median of --repeat calls after one warm-up call, and ms per iteration.  The split by kernel comes from a
kernel trace of one such run (rocprofv3 --kernel-trace --stats -- python scripts/bench_quantify.py --repeat 1).
--reference N times N iterations of the reference's own EM_trans / EM_meta loop, restated in Python with its data structures, on the same
problem on the CPU this runs on (seconds per iteration; --reference-only: without a GPU).

    python scripts/bench_quantify.py [--scale 1.0] [--repeat 3] [--reference N] [--reference-only]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nanosim_amd import characterize, engine      # noqa: E402


def problem(kind: str, n_targets: int, n_reads: int, seed: int) -> dict:
    """an em_problem in array form, built without Python dicts (2*10^6 keys would only measure the dict)"""
    rng = np.random.default_rng(seed)
    expr = rng.gamma(0.5, 1.0, n_targets)
    expr[rng.random(n_targets) < 0.1] = 0.0                 # unexpressed targets: the threshold is 0
    expr /= expr.sum()
    first = rng.choice(n_targets, size=n_reads, p=expr).astype(np.uint32)
    length = rng.integers(200, 5000, n_reads) if kind == "meta" else np.ones(n_reads, dtype=np.int64)
    multi = rng.random(n_reads) < 0.3
    unique = np.bincount(first[~multi], weights=length[~multi].astype(np.float64), minlength=n_targets)
    mf, ml = first[multi], length[multi]
    n_cand = rng.integers(2, 5 if kind == "trans" else 4, len(mf))
    multi_off = np.zeros(len(mf) + 1, dtype=np.uint64)
    np.cumsum(n_cand, out=multi_off[1:])
    target = np.repeat(mf, n_cand)
    pos = np.arange(len(target)) - np.repeat(multi_off[:-1].astype(np.int64), n_cand)
    target = ((target + pos * (1 + rng.integers(0, 5, len(target)))) % n_targets).astype(np.uint32)      # neighbours: isoforms, related species
    return dict(kind=kind, names=list(range(n_targets)), unique=unique, total=int(length.sum()), keys=range(len(mf)), multi_off=multi_off,
                target=target, weight=ml.astype(np.float64))


def reference_seconds(prob: dict, iterations: int) -> float:
    """EM_trans / EM_meta (G:60-84, G:104-127) restated with the reference's data structures: seconds per iteration on this CPU"""
    max_iter, factor, _ = characterize.EM_KINDS[prob["kind"]]
    max_iter = min(max_iter, iterations)
    names = prob["names"]
    off, tgt, w = prob["multi_off"].tolist(), prob["target"].tolist(), prob["weight"].tolist()
    multi = {m: tgt[off[m]:off[m + 1]] for m in range(len(w))}
    unique = dict(zip(names, prob["unique"].tolist()))
    total = prob["total"]
    t0 = time.perf_counter()
    a = {t: 100 / len(names) for t in names}
    diff = 100 * len(names)
    done = 0
    for _ in range(max_iter):
        done += 1
        cnt = {k: v for k, v in unique.items()}
        for m, cand in multi.items():
            tot = sum([a[c] for c in cand])
            perc = [a[c] / tot for c in cand]
            for i in range(len(cand)):
                cnt[cand[i]] += w[m] * perc[i]
        new = {t: c * 100 / total for t, c in cnt.items()}
        d = sum([abs(new[t] - a[t]) for t in a])
        a = new
        th = min(a.values()) * factor
        if d <= th or diff - d < th:
            break
        diff = d
    return (time.perf_counter() - t0) / done


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--reference", type=int, default=0)
    ap.add_argument("--reference-only", action="store_true")
    a = ap.parse_args()
    eng = None if a.reference_only else engine.Engine(0)
    try:
        for kind, n_targets, n_reads in (("trans", int(200000 * a.scale), int(2000000 * a.scale)), ("meta", 10, int(1000000 * a.scale))):
            prob = problem(kind, max(n_targets, 2), n_reads, 7)
            if eng is None:
                print(json.dumps({"metric": "reference EM loop, CPU seconds per iteration", "kind": kind, "targets": len(prob["names"]), "reads": n_reads,
                                  "iterations_timed": a.reference, "s_per_iteration": reference_seconds(prob, max(a.reference, 1))}), flush=True)
                continue
            characterize.em_call(eng, prob)                 # warm-up
            runs = [characterize.em_call(eng, prob) for _ in range(a.repeat)]
            ms = statistics.median(r["ms_kernel"] for r in runs)
            out = {"metric": "ns_em_quantify loop ms", "kind": kind, "targets": len(prob["names"]), "reads": n_reads, "multi": len(prob["weight"]),
                   "candidates": len(prob["target"]), "n_iter": runs[0]["n_iter"], "ms": ms, "ms_min": min(r["ms_kernel"] for r in runs),
                   "ms_per_iteration": ms / runs[0]["n_iter"], "repeat": a.repeat}
            if a.reference:
                out["reference_cpu_s_per_iteration"] = reference_seconds(prob, a.reference)
            print(json.dumps(out), flush=True)
    finally:
        if eng is not None:
            eng.close()


if __name__ == "__main__":
    main()
