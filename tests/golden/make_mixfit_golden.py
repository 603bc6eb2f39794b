#!/usr/bin/env python3
"""Golden fixture of the training side's mixture fit: the REAL reference's src/model_fitting.py (F:) and src/mixed_model.py
are imported unmodified in the build container; the module globals are set the way model_fitting() sets them (F:111-114) and mis_fit /
ins_fit / del_fit, mis_ll / ins_ll / del_ll and read_histogram are called directly.  What they return is committed as data.

 (a) three histograms of 20 000 seeded draws each from mixed_model.pois_geom(0.6, 0.7, 0.4), wei_geom(1.1, 0.9, 0.5, 0.3) and
     wei_geom(1.4, 1.1, 0.6, 0.35): the CDFs read_histogram returns, EVERY start of the three grids (F:120-121, 153-154, 186-187) with
     the reference's x and residual, and the text of _model_profile of one unmodified model_fitting(prefix, cores) run with its wall time.
     Should the file pass 1 MB, the indel grids are kept at a stride of 7 plus their 64 best starts.
 (b) long tails: CDFs of 150 bins (mismatch) and 131 bins (indel) — more than two 64-bin tiles and no multiple of one — with 16 and 64
     starts spread over the grids.
 (c) the objective alone: mis_ll / ins_ll / del_ll at 200 seeded points per type, half on (a) and half on (b).  About a quarter are invalid
     (a zero or negative parameter, p > 1), some have w > 1 (the clip bites), some l = 1e-3, k = 5 (the power leaves exp's range), a few
     p = 1.  NaN is stored as NaN.

 (d) np.argsort, which orders scipy's simplex: its result for every pattern of four and of five values over three levels and NaN.  It is
     not a stable sort on this hardware, and the searches meet ties (csrc/ns_mixfit.h: MfSimplex::sort).

The grids take about ten minutes on 8 cores.  --cache FILE keeps the raw results of the slow part in a pickle so that the packing can be
repeated without them.

    python tests/golden/make_mixfit_golden.py        -> tests/golden/reference_mixfit.json.gz
"""
import argparse
import contextlib
import gzip
import io
import json
import multiprocessing as mp
import os
import pickle
import shutil
import sys
import tempfile
import time
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF_SRC = "/root/reference/src"
SEED_A, SEED_B, SEED_C = 20261019, 20261020, 20261021
N_DRAWS = 20000
LIMIT = 1000000


def hist_text(h, head):
    """the text hist() writes for a length histogram (rows 0 .. at least 29)"""
    n = max(30, max(h) + 1)
    return "number of bases\t%s:\n" % head + "".join("%d\t%d\n" % (k, h.get(k, 0)) for k in range(n))


def draw_hist(fn, args, n):
    h = {}
    for _ in range(n):
        v = int(fn(*args))
        h[v] = h.get(v, 0) + 1
    return h


def long_tail(rng, n_max, first):
    """a histogram whose lengths run from `first` to n_max: a geometric body and a thin tail that reaches the end"""
    h = {}
    for v in rng.geometric(0.12, size=N_DRAWS):
        v = int(v) + first - 1
        if v <= n_max:
            h[v] = h.get(v, 0) + 1
    for v in rng.integers(first, n_max + 1, size=400):
        h[int(v)] = h.get(int(v), 0) + 1
    h[n_max] = h.get(n_max, 0) + 1
    return h


def grids():
    a = np.arange
    mis = [(l, p, w) for l in a(0.1, 0.9, 0.1) for p in a(0.1, 0.9, 0.1) for w in a(0.1, 0.9, 0.1)]
    indel = [(l, p, k, w) for l in a(0.1, 1.3, 0.1) for p in a(0.1, 1.3, 0.1) for k in a(0.1, 0.9, 0.1) for w in a(0.1, 0.9, 0.1)]
    return mis, indel


def points(rng, n, dim):
    """n points of (l, p, w) or (l, k, p, w)"""
    out = []
    ip = 1 if dim == 3 else 2
    for i in range(n):
        x = [float(rng.uniform(0.05, 3.0))] + ([float(rng.uniform(0.1, 3.0))] if dim == 4 else []) + \
            [float(rng.uniform(0.01, 1.0)), float(rng.uniform(0.01, 0.99))]
        u = rng.random()
        if u < 0.25:                                   # invalid
            j = int(rng.integers(0, dim + 1))
            if j == dim:
                x[ip] = float(rng.uniform(1.0, 1.5)) + 1e-9
            else:
                x[j] = (0.0, -float(rng.uniform(0.01, 1.0)))[int(rng.integers(0, 2))]
        elif u < 0.35:
            x[-1] = float(rng.uniform(1.0, 1.6))       # the clip bites
        elif u < 0.42:
            x[0] = 1e-3
            if dim == 4:
                x[1] = 5.0
        elif u < 0.46:
            x[ip] = 1.0
        elif u < 0.50:
            x[0] = float(rng.uniform(20.0, 80.0))
        out.append(x)
    return out


def run_grid(fit, tasks, cores):
    pool = mp.Pool(cores)                              # forked: the children see the module globals set by the caller
    res = pool.map(fit, tasks, chunksize=8)
    pool.close()
    pool.join()
    return [([float(v) for v in r[1]], float(r[2])) for r in res]


def slow_part(F, cores):
    import mixed_model as M
    warnings.simplefilter("ignore")
    work = tempfile.mkdtemp(prefix="nsmf_")
    raw = {}
    try:
        # (a)
        np.random.seed(SEED_A)
        ha = dict(mis=draw_hist(M.pois_geom, (0.6, 0.7, 0.4), N_DRAWS), ins=draw_hist(M.wei_geom, (1.1, 0.9, 0.5, 0.3), N_DRAWS),
                  **{"del": draw_hist(M.wei_geom, (1.4, 1.1, 0.6, 0.35), N_DRAWS)})
        rng = np.random.default_rng(SEED_B)
        hb = dict(mis=long_tail(rng, 151, 1), indel=long_tail(rng, 132, 1))
        heads = dict(mis="Mismatches", ins="Insertions", indel="Insertions", **{"del": "Deletions"})
        for tag, hs in (("a", ha), ("b", hb)):
            for t, h in hs.items():
                with open(os.path.join(work, "%s_%s.hist" % (tag, t)), "w") as f:
                    f.write(hist_text(h, heads[t]))
        raw["hist_a"], raw["hist_b"] = ha, hb
        pa, pb = os.path.join(work, "a"), os.path.join(work, "b")
        os_a = {}
        cdf_a, cdf_b = {}, {}
        for t, e in (("mis", "mis"), ("ins", "indel"), ("del", "indel")):
            os_a[t], cdf_a[t] = F.read_histogram("%s_%s.hist" % (pa, t), e)
        for t in ("mis", "indel"):
            _, cdf_b[t] = F.read_histogram("%s_%s.hist" % (pb, t), t)
        assert len(cdf_b["mis"]) == 150 and len(cdf_b["indel"]) == 131
        raw["cdf_a"] = {t: [float(v) for v in c] for t, c in cdf_a.items()}
        raw["cdf_b"] = {t: [float(v) for v in c] for t, c in cdf_b.items()}
        raw["n_obs_a"] = {t: len(o) for t, o in os_a.items()}
        g_mis, g_indel = grids()

        # (c) first: it is quick
        rng = np.random.default_rng(SEED_C)
        obj = []
        for t, ll, name, dim in (("mis", F.mis_ll, "mis_cdf", 3), ("ins", F.ins_ll, "ins_cdf", 4), ("del", F.del_ll, "del_cdf", 4)):
            for tag, cdf in (("a", cdf_a[t]), ("b", cdf_b["mis" if t == "mis" else "indel"])):
                setattr(F, name, cdf)
                pts = points(rng, 100, dim)
                obj.append(dict(type=t, set=tag, points=pts, values=[float(ll(x)) for x in pts]))
        raw["objective"] = obj

        # (b)
        F.mis_cdf, F.ins_cdf = cdf_b["mis"], cdf_b["indel"]
        t0 = time.time()
        F.mis_fit(g_mis[77])
        print("(b) one mismatch start: %.1f s" % (time.time() - t0), flush=True)
        ib_mis = [int(i) for i in np.linspace(0, len(g_mis) - 1, 16).round()]
        ib_ind = [int(i) for i in np.linspace(0, len(g_indel) - 1, 64).round()]
        raw["b"] = dict(mis=dict(index=ib_mis, res=run_grid(F.mis_fit, [g_mis[i] for i in ib_mis], cores)),
                        indel=dict(index=ib_ind, res=run_grid(F.ins_fit, [g_indel[i] for i in ib_ind], cores)))
        print("(b) done", flush=True)

        # (a): every start
        F.mis_cdf, F.ins_cdf, F.del_cdf = cdf_a["mis"], cdf_a["ins"], cdf_a["del"]
        F.mis_os, F.ins_os, F.del_os = os_a["mis"], os_a["ins"], os_a["del"]
        raw["a"] = {}
        for t, fit, g in (("mis", F.mis_fit, g_mis), ("ins", F.ins_fit, g_indel), ("del", F.del_fit, g_indel)):
            t0 = time.time()
            raw["a"][t] = run_grid(fit, g, cores)
            print("(a) %s: %d starts, %.0f s on %d cores" % (t, len(g), time.time() - t0, cores), flush=True)

        # one unmodified run
        t0 = time.time()
        with contextlib.redirect_stdout(io.StringIO()):
            F.model_fitting(pa, cores)
        raw["profile_wall_s"] = time.time() - t0
        raw["profile_cores"] = cores
        raw["profile"] = open(pa + "_model_profile").read()
        print("model_fitting: %.0f s on %d cores" % (raw["profile_wall_s"], cores), flush=True)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    return raw


def argsort_patterns():
    import itertools
    levels = (0.25, 0.5, 0.75, float("nan"))
    return [[list(v), [int(i) for i in np.argsort(np.array(v))]] for n in (4, 5) for v in itertools.product(levels, repeat=n)]


def pack(raw, thin):
    import scipy
    a = {}
    for t, res in raw["a"].items():
        idx = list(range(len(res)))
        if thin and t != "mis":
            best = sorted((i for i in idx if res[i][1] == res[i][1]), key=lambda i: (res[i][1], i))[:64]
            idx = sorted(set(idx[::7]) | set(best))
        a[t] = dict(n_starts=len(res), index=idx, x=[res[i][0] for i in idx], residual=[res[i][1] for i in idx])
    b = {t: dict(index=v["index"], x=[r[0] for r in v["res"]], residual=[r[1] for r in v["res"]]) for t, v in raw["b"].items()}
    return dict(versions=dict(scipy=scipy.__version__, numpy=np.__version__, python=sys.version.split()[0]),
                seeds=[SEED_A, SEED_B, SEED_C],
                a=dict(hist={t: sorted(h.items()) for t, h in raw["hist_a"].items()}, cdf=raw["cdf_a"], n_obs=raw["n_obs_a"], fits=a,
                       model_profile=raw["profile"], model_fitting_wall_s=raw["profile_wall_s"], model_fitting_cores=raw["profile_cores"]),
                b=dict(hist={t: sorted(h.items()) for t, h in raw["hist_b"].items()}, cdf=raw["cdf_b"], fits=b),
                objective=raw["objective"], argsort=argsort_patterns())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cache")
    ap.add_argument("--cores", type=int, default=8)
    args = ap.parse_args()
    sys.dont_write_bytecode = True
    if REF_SRC not in sys.path:
        sys.path.insert(0, REF_SRC)
    if args.cache and os.path.exists(args.cache):
        raw = pickle.load(open(args.cache, "rb"))
    else:
        import model_fitting as F
        raw = slow_part(F, args.cores)
        if args.cache:
            pickle.dump(raw, open(args.cache, "wb"))
    out = os.path.join(HERE, "reference_mixfit.json.gz")
    for thin in (False, True):
        with gzip.open(out, "wt", compresslevel=9) as f:
            json.dump(pack(raw, thin), f)
        if os.path.getsize(out) < LIMIT:
            break
    print("written", out, os.path.getsize(out), "bytes; indel grids", "thinned" if thin else "whole")


if __name__ == "__main__":
    main()
