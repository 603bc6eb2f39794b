"""The engine's scalar primitives, evaluated directly: ns_log, ns_exp, ns_norminv (Acklam), ns_pow10m1, u53_to_p, the integer
thresholds ns_thr_lt / ns_thr_gt, ecdf_lookup, table_value, trans_pick_u and the saturating conversion ns_f64_to_i64_sat / ns_len_draw
(nanosim_amd/csrc/ns_rng.h, ns_device.h).  tests/math_probe.hip compiles them for gfx950 (one kernel per primitive) and for the host; the
oracle's copies (oracle/ns_oracle.c nso_eval_batch) are the reference.  The bit-exact design rests on these giving
the same bits on both targets; the whole-batch parity tests reach them only through the draws a few thousand reads make (the norminv tails
below p = 2^-20 about once in 10^6 draws).

What is asserted:
  - GPU == host build == oracle, bit for bit, on every input of the grids below (the GPU half is marked gpu);
  - accuracy against mpmath at 50 digits on a subsample of ~20 000 points that holds every edge point (bounds at ACCURACY);
  - norminv(u32_to_p(u)) non-decreasing in u: over all 2^32 u on the GPU (a reduction kernel), over the tails and the break points on the CPU;
  - for every t and u of the threshold grid: u < ns_thr_lt(t) <=> u32_to_p(u) < t, and u >= ns_thr_gt(t) <=> u32_to_p(u) > t;
  - ns_f64_to_i64_sat is C's truncation wherever that is defined, saturates outside the int64 range and gives 0 for NaN."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not found")

OP_LOG, OP_EXP, OP_NORMINV_U, OP_POW10M1, OP_U53, OP_THR_LT, OP_THR_GT, OP_F64_I64, OP_NORMINV, OP_LEN_DRAW = range(10)
NAMES = {OP_LOG: "ns_log", OP_EXP: "ns_exp", OP_NORMINV_U: "ns_norminv(u32_to_p(u))", OP_POW10M1: "ns_pow10m1", OP_U53: "u53_to_p",
         OP_THR_LT: "ns_thr_lt", OP_THR_GT: "ns_thr_gt", OP_F64_I64: "ns_f64_to_i64_sat", OP_NORMINV: "ns_norminv", OP_LEN_DRAW: "ns_len_draw"}
CHUNK = 1 << 22
LEN_DRAW_MAX = 0x3fffffff
PLOW = 0.02425
# Accuracy bounds against mpmath (50 digits):
#   ns_log      |err| <= 4e-16 max(1, |log x|)                     (as test_oracle_pin.test_exact_math_accuracy), normal x
#   ns_exp      |err| <= 1e-15 exp(y), y in [-700, 700]; outside: the value at the clamp
#   ns_norminv  |err| <= 1.15e-9 max(1, |z|) (Acklam's relative error of the approximation), p down to 2^-33 (u = 0 gives p = 2^-33)
#   ns_pow10m1  |err| <= 4e-16 + 1e-13 10^x: absolute near 0 (exp(x ln 10) - 1 cancels), relative for large x
ACCURACY = dict(log=4e-16, exp=1e-15, norminv=1.15e-9, pow10m1_abs=4e-16, pow10m1_rel=1e-13)


def _hipcc():
    return HIPCC if os.path.exists(HIPCC) else "hipcc"


def _load(path):
    L = C.CDLL(path)
    L.probe_gpu.restype = C.c_int; L.probe_gpu.argtypes = []
    L.probe_eval.restype = C.c_int; L.probe_eval.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint64]
    L.probe_ecdf.restype = C.c_int
    L.probe_ecdf.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_double, C.c_void_p, C.c_void_p, C.c_uint64]
    L.probe_table_value.restype = C.c_int
    L.probe_table_value.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64]
    L.probe_trans_pick.restype = C.c_int; L.probe_trans_pick.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
    return L


def build_probe(tmp, gpu):
    """tests/math_probe.hip for the host (--cuda-host-only -DNS_HOST_TEST, as tests/test_chain_host.py) or for gfx950 with the engine's
    flags (__graft_entry__.HIP_FLAGS), into tmp."""
    src = os.path.join(ROOT, "tests", "math_probe.hip")
    if gpu:
        import __graft_entry__ as G
        out = os.path.join(tmp, "math_probe_gfx950.so")
        cmd = [_hipcc()] + G.HIP_FLAGS + ["-o", out, src]
    else:
        out = os.path.join(tmp, "math_probe_host.so")
        cmd = [_hipcc(), "--cuda-host-only", "-x", "hip", "-O3", "-std=c++17", "-ffp-contract=off", "-DNS_HOST_TEST", "-shared", "-fPIC",
               "-o", out, src]
    subprocess.check_call(cmd, cwd=ROOT)
    L = _load(out)
    assert L.probe_gpu() == (1 if gpu else 0)
    return L


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_probe(str(tmp_path_factory.mktemp("math_probe_host")), gpu=False)


# ---- evaluation ------------------------------------------------------------------------------------------------------------------
def _bits(x):
    """8-byte input elements: float64 arrays as their bits, integer arrays as uint64"""
    a = np.ascontiguousarray(x)
    return a.view(np.uint64) if a.dtype == np.float64 else a.astype(np.uint64)


def probe_eval(L, op, x):
    x = _bits(x)
    out = np.empty(len(x), dtype=np.uint64)
    for s in range(0, len(x), CHUNK):
        xi = np.ascontiguousarray(x[s:s + CHUNK]); oi = np.empty(len(xi), dtype=np.uint64)
        assert L.probe_eval(op, xi.ctypes.data, oi.ctypes.data, len(xi)) == 0, NAMES[op]
        out[s:s + len(xi)] = oi
    return out


def oracle_eval(op, x):
    x = _bits(x)
    out = np.empty(len(x), dtype=np.uint64)
    assert O.lib().nso_eval_batch(op, x.ctypes.data, out.ctypes.data, len(x)) == 0
    return out


def assert_same_bits(a, b, op, x, what):
    bad = np.nonzero(a != b)[0]
    if len(bad):
        i = bad[0]
        xb = _bits(x)[i]
        raise AssertionError("%s: %s differs on %d of %d inputs; first: input bits %#x -> %#x against %#x"
                             % (NAMES[op], what, len(bad), len(a), int(xb), int(a[i]), int(b[i])))


def as_f64(bits):
    return bits.view(np.float64)


# ---- input grids -----------------------------------------------------------------------------------------------------------------
def _ulps(x, k):
    """x and its k nearest neighbours on either side (float64)"""
    x = np.atleast_1d(np.asarray(x, dtype=np.float64))
    out = [x]
    up, dn = x.copy(), x.copy()
    with np.errstate(over="ignore"):
        for _ in range(k):
            up = np.nextafter(up, np.inf); dn = np.nextafter(dn, -np.inf)
            out += [up, dn]
    return np.concatenate(out)


def norminv_u_grid():
    """every u in the two tails [0, 2^24) and [2^32 - 2^24, 2^32), every 257th u over the full range, and the u around the break points"""
    brk = [int(PLOW * 2.0 ** 32), int((1.0 - PLOW) * 2.0 ** 32)]
    return np.concatenate([np.arange(0, 1 << 24, dtype=np.uint64), np.arange((1 << 32) - (1 << 24), 1 << 32, dtype=np.uint64),
                           np.arange(0, 1 << 32, 257, dtype=np.uint64)] +
                          [np.arange(b - 4096, b + 4096, dtype=np.uint64) for b in brk])


def norminv_p_grid():
    """p within +-64 ulps of the break points 0.02425 and 1 - 0.02425 (no u lands there: its p are 2^-32 apart), p = 2^-33 .. 1 - 2^-33"""
    return np.concatenate([_ulps(PLOW, 64), _ulps(1.0 - PLOW, 64), _ulps(0.5, 16), _ulps(2.0 ** -33, 8), _ulps(1.0 - 2.0 ** -33, 8)])


def log_grid():
    """every binary exponent of a positive finite double (subnormals included; the callers reach 2^-33 .. 2^64), the mantissa edges
    around sqrt(2) (the reduction's switch), 1 and 2, and random mantissas per exponent"""
    rng = np.random.default_rng(11)
    e = np.arange(-1022, 1024, dtype=np.float64)
    m = np.concatenate([_ulps(1.0, 4), _ulps(math.sqrt(2.0), 32), _ulps(np.nextafter(2.0, 0), 4)[1:], [1.25, 1.5, 1.75]])
    m = m[(m >= 1.0) & (m < 2.0)]
    grid = (np.ldexp(m[:, None], e[None, :].astype(np.int64))).ravel()
    rnd = np.ldexp(rng.uniform(1.0, 2.0, (len(e), 16)), e[:, None].astype(np.int64)).ravel()
    sub = np.ldexp(np.concatenate([[1.0], rng.uniform(1.0, 2.0, 64)]), rng.integers(-1074, -1023, 65))
    return np.concatenate([grid, rnd, sub, [0.0, 5e-324, np.nextafter(2.0 ** -1022, 0)]])


def exp_grid():
    """y across the +-700 clamps and up to +-800, every point where k = floor(fma(y, log2 e, 0.5)) changes (with +-4 ulps), dense random"""
    rng = np.random.default_rng(12)
    k = np.arange(-1011, 1011, dtype=np.float64)
    steps = (k - 0.5) / 1.4426950408889634
    steps = steps[np.abs(steps) <= 700.0]
    return np.concatenate([_ulps(steps, 4), _ulps([700.0, -700.0], 64), np.linspace(-800, 800, 16001), rng.uniform(-700, 700, 200000),
                           _ulps(0.0, 8), [1e-300, -1e-300, 1e300, -1e300]])


def pow10m1_grid():
    """x over [-1, 8] (the head/tail, gap lengths are log10 values), dense near 0"""
    rng = np.random.default_rng(13)
    tiny = np.concatenate([10.0 ** -np.arange(1, 300, dtype=np.float64), 2.0 ** -np.arange(1, 1000, dtype=np.float64)])
    return np.concatenate([np.linspace(-1, 8, 180001), rng.uniform(-1, 8, 100000), tiny, -tiny, rng.uniform(-1e-6, 1e-6, 20000),
                           _ulps(0.0, 8)])


def threshold_grid():
    """t at k 2^-32, (k +- 0.5) 2^-32 and their nextafter neighbours, for k at both ends and random; 0, 1, subnormals, out of [0, 1]"""
    rng = np.random.default_rng(14)
    k = np.concatenate([np.arange(0, 1025), np.arange((1 << 32) - 1024, (1 << 32) + 1), rng.integers(0, 1 << 32, 20000)]).astype(np.float64)
    base = np.concatenate([k, k + 0.5, k - 0.5]) * 2.0 ** -32
    base = base[(base >= 0.0) & (base <= 1.0)]
    extra = np.array([0.0, -0.0, 1.0, 5e-324, 2.0 ** -1022, 2.0 ** -1074 * 7, -1e-300, -0.5, 1.5, 2.0 ** -33, 1.0 - 2.0 ** -33])
    return np.concatenate([_ulps(base, 1), _ulps(extra, 2)])


def conversion_grid():
    """NaN, +-inf, +-2^63, +-2^31, 2^30 and their neighbours, 1e19, 1e304, fractions, random over the whole exponent range"""
    rng = np.random.default_rng(15)
    edges = [2.0 ** 63, -2.0 ** 63, 2.0 ** 31, -2.0 ** 31, 2.0 ** 31 - 1, -2.0 ** 31 - 1, 2.0 ** 30, 2.0 ** 30 - 1, 2.0 ** 32,
             0.0, 0.5, -0.5, 1.0, -1.0, 1e19, -1e19, 1e304, -1e304, 1.7976931348623157e308, -1.7976931348623157e308]
    rnd = np.ldexp(rng.uniform(-2.0, 2.0, 40000), rng.integers(-60, 80, 40000))
    return np.concatenate([_ulps(edges, 8), [np.inf, -np.inf, np.nan, -np.nan, -0.0], rnd])


def u53_grid():
    rng = np.random.default_rng(16)
    a = rng.integers(0, 1 << 32, 200000, dtype=np.uint64); b = rng.integers(0, 1 << 32, 200000, dtype=np.uint64)
    e = np.array([0, 0x1f, 0x20, 0x3f, 0x40, 0xffffffc0, 0xffffffdf, 0xffffffe0, 0xffffffff], dtype=np.uint64)
    ea, eb = np.meshgrid(e, e)
    return np.concatenate([(a << np.uint64(32)) | b, (ea.ravel() << np.uint64(32)) | eb.ravel()])


GRIDS = [(OP_NORMINV_U, norminv_u_grid), (OP_NORMINV, norminv_p_grid), (OP_LOG, log_grid), (OP_EXP, exp_grid), (OP_POW10M1, pow10m1_grid),
         (OP_U53, u53_grid), (OP_THR_LT, threshold_grid), (OP_THR_GT, threshold_grid), (OP_F64_I64, conversion_grid),
         (OP_LEN_DRAW, conversion_grid)]


@pytest.fixture(scope="module")
def oracle_results():
    """the oracle's value on every grid, once per module: {op: (inputs, outputs)}"""
    res = {}
    for op, grid in GRIDS:
        x = grid()
        res[op] = (x, oracle_eval(op, x))
    return res


# ---- host build == oracle (every CPU run) -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", [g[0] for g in GRIDS], ids=[NAMES[g[0]] for g in GRIDS])
def test_host_build_matches_oracle(host, oracle_results, op):
    x, exp = oracle_results[op]
    assert_same_bits(probe_eval(host, op, x), exp, op, x, "host build against the oracle")


def _small_model():
    from nanosim_amd import model
    return model.load_model(os.path.join(ROOT, "tests", "golden", "model_small", "training"), chimeric=True, homopolymer=True, fastq=True)


def _table_cases(m):
    """(hi, vhi, vlo0) of every ECDF column of the small model, the inverse-CDF tables, the transition rows"""
    cols = [m.first_match] + list(m.match_markov)
    ecdf = [(np.ascontiguousarray(c.hi, dtype=np.float64), np.ascontiguousarray(c.vhi, dtype=np.float64), float(c.vlo0)) for c in cols]
    cdfs = [np.ascontiguousarray(m.nseg_cdf, dtype=np.float64)] if getattr(m, "nseg_cdf", None) is not None else []
    for t in m.mix_cdf if getattr(m, "mix_cdf", None) is not None else []:
        for c in t:
            cdfs.append(np.ascontiguousarray(c, dtype=np.float64))
    return ecdf, [c for c in cdfs if len(c)], np.asarray(m.trans, dtype=np.float64)


def _edge_ps(edges, rng, n=3000):
    edges = np.asarray(edges, dtype=np.float64)
    return np.ascontiguousarray(np.concatenate([rng.uniform(0, 1, n), edges, np.nextafter(edges, 2), np.nextafter(edges, -1),
                                                [0.0, 1e-300, 2.0 ** -33, 1.0 - 2.0 ** -33, 1.0]]))


def _trans_u(row, rng):
    """draws around the two thresholds of a transition row, at both ends and random"""
    t = [O_thr_lt(row[0]), O_thr_lt(row[1])]
    near = np.concatenate([np.arange(max(0, v - 3), min(1 << 32, v + 4)) for v in t])
    return np.ascontiguousarray(np.concatenate([near, [0, 1, 0xfffffffe, 0xffffffff], rng.integers(0, 1 << 32, 5000)]).astype(np.uint32))


def O_thr_lt(t):
    return int(oracle_eval(OP_THR_LT, np.array([t], dtype=np.float64))[0])


def table_results(L):
    """ecdf_lookup, table_value, trans_pick_u of probe library L against the oracle's nso_ecdf_lookup / nso_table_value / nso_trans_pick
    (the fp64 compares the integer thresholds stand for) on the small model's tables; returns the number of points checked"""
    Lo = O.lib()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    rng = np.random.default_rng(17)
    ecdf, cdfs, trans = _table_cases(_small_model())
    n = 0
    for hi, vhi, vlo0 in ecdf:
        p = _edge_ps(hi, rng)
        got = np.empty(len(p), dtype=np.int64)
        assert L.probe_ecdf(hi.ctypes.data, vhi.ctypes.data, len(hi), vlo0, p.ctypes.data, got.ctypes.data, len(p)) == 0
        exp = np.array([Lo.nso_ecdf_lookup(dp(hi), dp(vhi), len(hi), vlo0, float(q)) for q in p], dtype=np.int64)
        assert np.array_equal(got, exp), ("ecdf_lookup", np.nonzero(got != exp)[0][:5])
        n += len(p)
    assert cdfs, "the small model has inverse-CDF tables"
    for cdf in cdfs:
        p = _edge_ps(cdf, rng)
        got = np.empty(len(p), dtype=np.int64)
        assert L.probe_table_value(cdf.ctypes.data, len(cdf), p.ctypes.data, got.ctypes.data, len(p)) == 0
        exp = np.array([Lo.nso_table_value(dp(cdf), len(cdf), float(q)) for q in p], dtype=np.int64)
        assert np.array_equal(got, exp), ("table_value", np.nonzero(got != exp)[0][:5])
        n += len(p)
    for row in trans:
        thr = np.array([O_thr_lt(row[0]), O_thr_lt(row[1])], dtype=np.uint64)     # T0, T1 as ns_pack builds them
        u = _trans_u(row, rng)
        got = np.empty(len(u), dtype=np.int32)
        assert L.probe_trans_pick(thr.ctypes.data, u.ctypes.data, got.ctypes.data, len(u)) == 0
        crow = (C.c_double * 3)(*row)
        p = (u.astype(np.float64) + 0.5) * 2.0 ** -32
        exp = np.array([Lo.nso_trans_pick(crow, float(q)) for q in p], dtype=np.int32)
        assert np.array_equal(got, exp), ("trans_pick_u", row, np.nonzero(got != exp)[0][:5])
        n += len(u)
    return n


def test_host_tables_match_oracle(host):
    assert table_results(host) > 10000


# ---- properties of the oracle's (== the host build's) values -----------------------------------------------------------------------
def test_norminv_monotone_tails_and_breaks(oracle_results):
    """norminv(u32_to_p(u)) non-decreasing over each contiguous run of u of the grid: both 2^24 tails and the break points"""
    x, y = oracle_results[OP_NORMINV_U]
    z = as_f64(y)
    n257 = len(range(0, 1 << 32, 257))
    runs = [(0, 1 << 24), (1 << 24, 2 << 24), (2 << 24, (2 << 24) + n257)]
    off = (2 << 24) + n257
    runs += [(off, off + 8192), (off + 8192, off + 16384)]
    for a, b in runs:
        assert np.all(np.diff(x[a:b].astype(np.int64)) > 0)                    # (the run is increasing in u)
        d = np.diff(z[a:b])
        assert np.all(d >= 0), ("norminv decreases at u = %d" % int(x[a + int(np.argmax(d < 0)) + 1]))
    p = norminv_p_grid()
    o = np.argsort(p, kind="stable")
    zp = as_f64(oracle_results[OP_NORMINV][1])[o]
    # p one ulp apart: the formula's rounding wiggles by ~1e-13 (1 - p, (p - 0.5)^2), far below the step between two draws (~4e-9 here),
    # so monotone in u (above) and within 1e-12 from one p to the next across the break points
    assert np.all(np.diff(zp) >= -1e-12), "norminv steps down across a break point"


def test_threshold_equivalence(oracle_results):
    """u < ns_thr_lt(t) <=> u32_to_p(u) < t and u >= ns_thr_gt(t) <=> u32_to_p(u) > t, for every t of the grid and the u around t 2^32"""
    t, lt = oracle_results[OP_THR_LT]
    _, gt = oracle_results[OP_THR_GT]
    assert np.all(lt <= (1 << 32)) and np.all(gt <= (1 << 32))
    k = np.floor(np.clip(t, 0.0, 1.0) * 2.0 ** 32)
    for d in range(-3, 4):
        u = np.clip(k + d, 0, 2.0 ** 32 - 1).astype(np.uint64)
        p = (u.astype(np.float64) + 0.5) * 2.0 ** -32                          # exact: u + 0.5 needs 33 bits
        assert np.array_equal(u < lt, p < t), "ns_thr_lt"
        assert np.array_equal(u >= gt, p > t), "ns_thr_gt"


def _spec_sat(x):
    if math.isnan(x):
        return 0
    if x >= 2.0 ** 63:
        return 2 ** 63 - 1
    if x < -2.0 ** 63:
        return -2 ** 63
    return int(x)                     # Python int(): truncation towards zero, exact for every double


def test_conversion_helper(oracle_results):
    """nso_f64_to_i64_sat / ns_f64_to_i64_sat: truncation where C defines it, saturation outside int64, NaN -> 0; ns_len_draw: -1 above
    0x3fffffff.  The edges by name: NaN, +-inf, +-2^63 and +-2^31 and their neighbours"""
    x, y = oracle_results[OP_F64_I64]
    got = y.view(np.int64)
    exp = np.array([_spec_sat(float(v)) for v in x], dtype=np.int64)
    assert np.array_equal(got, exp)
    _, yl = oracle_results[OP_LEN_DRAW]
    expl = np.where(exp > LEN_DRAW_MAX, -1, exp)
    assert np.array_equal(yl.view(np.int64), expl)
    L = O.lib()
    n63 = np.nextafter(2.0 ** 63, 0)
    for v, e in ((float("nan"), 0), (float("inf"), 2 ** 63 - 1), (float("-inf"), -2 ** 63), (2.0 ** 63, 2 ** 63 - 1), (n63, int(n63)),
                 (-2.0 ** 63, -2 ** 63), (np.nextafter(-2.0 ** 63, -np.inf), -2 ** 63), (np.nextafter(-2.0 ** 63, 0), int(np.nextafter(-2.0 ** 63, 0))),
                 (2.0 ** 31, 2 ** 31), (np.nextafter(2.0 ** 31, 0), 2 ** 31 - 1), (-2.0 ** 31, -2 ** 31),
                 (np.nextafter(-2.0 ** 31, -np.inf), -2 ** 31), (1e19, 2 ** 63 - 1), (-1e19, -2 ** 63), (1e304, 2 ** 63 - 1), (-0.9, 0)):
        assert L.nso_f64_to_i64_sat(float(v)) == e, v


# ---- accuracy against mpmath ------------------------------------------------------------------------------------------------------
def _subsample(x, n, edges, seed):
    rng = np.random.default_rng(seed)
    pick = x[rng.choice(len(x), size=min(n, len(x)), replace=False)]
    return np.unique(np.concatenate([pick, np.asarray(edges, dtype=x.dtype)]))


def test_accuracy_against_mpmath():
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    checked = 0
    # log: normal x over the exponents the callers reach (2^-40 .. 2^80) and the mantissa edges of every exponent in that range
    x = log_grid()
    x = x[(x >= 2.0 ** -40) & (x <= 2.0 ** 80)]
    xs = _subsample(x, 5000, np.concatenate([_ulps(math.sqrt(2.0), 32), _ulps(1.0, 4)[1:], np.ldexp(_ulps(math.sqrt(2.0), 2), -34)]), 1)
    got = as_f64(oracle_eval(OP_LOG, xs))
    for v, g in zip(xs, got):
        ref = mp.log(mp.mpf(float(v)))
        assert abs(mp.mpf(float(g)) - ref) <= ACCURACY["log"] * max(1.0, abs(float(ref))), ("ns_log", float(v))
    checked += len(xs)
    # exp: y in [-700, 700] including every step of k near the ends and the clamps; beyond them the value at the clamp
    y = exp_grid()
    ys = _subsample(y, 5000, np.concatenate([_ulps([700.0, -700.0], 4), [800.0, -800.0, 0.0]]), 2)
    got = as_f64(oracle_eval(OP_EXP, ys))
    for v, g in zip(ys, got):
        ref = mp.exp(mp.mpf(min(700.0, max(-700.0, float(v)))))
        assert abs(mp.mpf(float(g)) / ref - 1) <= ACCURACY["exp"], ("ns_exp", float(v))
    checked += len(ys)
    # norminv: u of both tails (p = 2^-33 at u = 0), the break points, the body
    u = norminv_u_grid()
    us = _subsample(u, 5000, np.array([0, 1, 2, 3, 255, 256, (1 << 24) - 1, (1 << 32) - 1, (1 << 32) - 2, 1 << 31, (1 << 31) - 1],
                                      dtype=np.uint64), 3)
    got = as_f64(oracle_eval(OP_NORMINV_U, us))
    pe = norminv_p_grid()
    gotp = as_f64(oracle_eval(OP_NORMINV, pe))
    for pv, g in list(zip(((us.astype(np.float64) + 0.5) * 2.0 ** -32), got)) + list(zip(pe, gotp)):
        ref = mp.sqrt(2) * mp.erfinv(2 * mp.mpf(float(pv)) - 1)
        assert abs(mp.mpf(float(g)) - ref) <= ACCURACY["norminv"] * max(1.0, abs(float(ref))), ("ns_norminv", float(pv))
    checked += len(us) + len(pe)
    # pow10m1: [-1, 8], dense near 0
    x = pow10m1_grid()
    xs = _subsample(x, 5000, np.concatenate([[-1.0, 0.0, 8.0, 1e-300, -1e-300], _ulps(0.0, 4)]), 4)
    got = as_f64(oracle_eval(OP_POW10M1, xs))
    for v, g in zip(xs, got):
        ref = mp.power(10, mp.mpf(float(v))) - 1
        assert abs(mp.mpf(float(g)) - ref) <= ACCURACY["pow10m1_abs"] + ACCURACY["pow10m1_rel"] * 10.0 ** float(v), ("ns_pow10m1", float(v))
    checked += len(xs)
    assert checked >= 20000


# ---- the GPU half ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu(tmp_path_factory):
    return build_probe(str(tmp_path_factory.mktemp("math_probe_gfx950")), gpu=True)


@pytest.mark.gpu
@pytest.mark.parametrize("op", [g[0] for g in GRIDS], ids=[NAMES[g[0]] for g in GRIDS])
def test_gpu_matches_host_and_oracle(gpu, host, oracle_results, op):
    x, exp = oracle_results[op]
    got = probe_eval(gpu, op, x)
    assert_same_bits(got, exp, op, x, "gfx950 against the oracle")
    assert_same_bits(got, probe_eval(host, op, x), op, x, "gfx950 against the host build")


@pytest.mark.gpu
def test_gpu_tables_match_oracle(gpu):
    assert table_results(gpu) > 10000


@pytest.mark.gpu
def test_gpu_norminv_monotone_all_u(gpu):
    """norminv(u32_to_p(u)) non-decreasing over all 2^32 u (one reduction kernel)"""
    gpu.probe_norminv_monotone.restype = C.c_int
    gpu.probe_norminv_monotone.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    n_bad, first = C.c_uint64(), C.c_uint64()
    assert gpu.probe_norminv_monotone(C.byref(n_bad), C.byref(first)) == 0
    assert n_bad.value == 0, "norminv decreases at %d u, first at u = %d" % (n_bad.value, first.value)
