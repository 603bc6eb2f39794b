"""What tests/test_mixfit.py (CPU) and tests/test_gpu_zzzzzzz_mixfit.py share: the reference's fixture
(tests/golden/reference_mixfit.json.gz, tests/golden/make_mixfit_golden.py) and the engine's mixture fit compiled for the host
(tests/mixfit_host.cpp: nanosim_amd/csrc/ns_mixfit.h as a wavefront of k_mixfit runs it, one thread walking the 64 lanes)."""
import ctypes as C
import gzip
import json
import os
import shutil
import subprocess
import types

import numpy as np

from nanosim_amd import characterize, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
TMP = os.path.join(ROOT, "tests", "_tmp")
HOST_FLAGS = ["--cuda-host-only", "-x", "hip", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread"]
MAXFEV_START = 510                   # the mismatch start (0.8, 0.8, 0.7): on set (a) it uses all 600 evaluations (status 1)
NAN_START = [0.5, 0.5, 1.2, 0.5]     # (l, k, p, w) with p > 1: every vertex of the first simplex is NaN
_cache = {}


def hipcc():
    return HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")


def load_fixture():
    if "fx" not in _cache:
        with gzip.open(os.path.join(ROOT, "tests", "golden", "reference_mixfit.json.gz"), "rt") as f:
            _cache["fx"] = json.load(f)
    return _cache["fx"]


def compile_host(out_name, extra):
    os.makedirs(TMP, exist_ok=True)
    out = os.path.join(TMP, out_name)
    subprocess.check_call([hipcc()] + HOST_FLAGS + extra + ["-o", out, os.path.join(ROOT, "tests", "mixfit_host.cpp")])
    return out


def build_host():
    """an object that stands in for an Engine: its ns_mixture_fit is ns_mixfit.h compiled for the host; .hand runs the hand cases"""
    if "host" in _cache:
        return _cache["host"]
    L = C.CDLL(compile_host("libmixfit_host.so", ["-fPIC", "-shared"]))
    L.mixfit_host_fit.restype = C.c_int
    L.mixfit_host_fit.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p]
    L.mixfit_host_hand.restype = C.c_int
    L.mixfit_host_hand.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]

    L.mixfit_host_argsort.restype = C.c_int
    L.mixfit_host_argsort.argtypes = [C.c_int, C.c_void_p, C.c_void_p]

    def argsort(values):
        v = np.ascontiguousarray(values, dtype=np.float64)
        order = np.zeros(len(v), dtype=np.uint32)
        assert L.mixfit_host_argsort(len(v), v.ctypes.data, order.ctypes.data) == 0
        return [int(i) for i in order]

    def check(rc):
        if rc:
            raise engine.EngineError("host mixture fit: error %d" % rc)

    def hand(which, x0, maxiter, maxfev):
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        r = characterize.NsMixfitFit()
        assert L.mixfit_host_hand(which, len(x0), x0.ctypes.data, maxiter, maxfev, C.byref(r)) == 0
        return r
    _cache["host"] = types.SimpleNamespace(ctx=None, L=types.SimpleNamespace(ns_mixture_fit=L.mixfit_host_fit), _check=check, hand=hand, argsort=argsort)
    return _cache["host"]


def fixture_sets(fx):
    """[(name, error, cdf, starts, reference x, reference residual)] of the fixture's five grids: (a) mis / ins / del — every start, or the
    stored ones of a thinned grid — and (b) mis / indel"""
    grids = {e: characterize.fit_starts(e) for e in ("mis", "indel")}
    out = []
    for t in ("mis", "ins", "del"):
        e = "mis" if t == "mis" else "indel"
        f = fx["a"]["fits"][t]
        assert f["n_starts"] == len(grids[e])
        out.append(("a/" + t, e, np.array(fx["a"]["cdf"][t]), grids[e][f["index"]], np.array(f["x"]), np.array(f["residual"]), np.array(f["index"])))
    for e in ("mis", "indel"):
        f = fx["b"]["fits"][e]
        out.append(("b/" + e, e, np.array(fx["b"]["cdf"][e]), grids[e][f["index"]], np.array(f["x"]), np.array(f["residual"]), np.array(f["index"])))
    return out


def host_fits(fx):
    """the host build's searches over fixture_sets, computed once per process: {name: mixture_fit's dict}"""
    if "fits" not in _cache:
        host = build_host()
        _cache["fits"] = {name: characterize.mixture_fit(host, e, cdf, starts) for name, e, cdf, starts, _, _, _ in fixture_sets(fx)}
    return _cache["fits"]


def objective_cdf(fx, entry):
    t = entry["type"]
    return np.array(fx["a"]["cdf"][t] if entry["set"] == "a" else fx["b"]["cdf"]["mis" if t == "mis" else "indel"])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
