"""Training side, the error-length mixtures on CPU: the engine's objectives and its Nelder-Mead search
(nanosim_amd/csrc/ns_mixfit.h, compiled for the host by tests/mixfit_host.cpp; on the GPU a wavefront of k_mixfit runs it per start) and
the host module around the call — pinned against what the REAL src/model_fitting.py returned for the same histograms
(tests/golden/reference_mixfit.json.gz, tests/golden/make_mixfit_golden.py) and, for the search skeleton, against scipy itself."""
import ctypes as C
import math
import os
import shutil
import subprocess
import warnings

import numpy as np
import pytest

from nanosim_amd import characterize, engine, model
from tests import mixfit_lib as ML

ROOT = ML.ROOT
pytestmark = pytest.mark.skipif(not ML.hipcc(), reason="hipcc not found")


@pytest.fixture(scope="module")
def fx():
    return ML.load_fixture()


@pytest.fixture(scope="module")
def host():
    return ML.build_host()


def as_hist(pairs):
    return {int(k): int(v) for k, v in pairs}


def reference_cdf(hist, error):
    """read_histogram's two numpy calls on the list of observations (F:34-43), for the corner cases"""
    obs = [k - (1 if error == "mis" else 0) for k, v in hist.items() for _ in range(v)]
    pmf, _ = np.histogram(obs, bins=max(obs) if error == "mis" else max(obs) - 1, density=True)
    return np.cumsum(pmf), len(obs)


# ---- the empirical CDF -------------------------------------------------------------------------------------------------------------------
def test_empirical_cdf_equals_the_fixture(fx):
    for t, e in (("mis", "mis"), ("ins", "indel"), ("del", "indel")):
        cdf, n = characterize.empirical_cdf(as_hist(fx["a"]["hist"][t]), e)
        assert np.array_equal(cdf, np.array(fx["a"]["cdf"][t])) and n == fx["a"]["n_obs"][t] == 20000
    for e, bins in (("mis", 150), ("indel", 131)):
        cdf, _ = characterize.empirical_cdf(as_hist(fx["b"]["hist"][e]), e)
        assert len(cdf) == bins and np.array_equal(cdf, np.array(fx["b"]["cdf"][e]))


def test_empirical_cdf_corners():
    for hist, e in (({3: 5, 4: 3, 7: 2, 9: 0}, "indel"), ({4: 2, 5: 7, 6: 1}, "mis"),       # the smallest length is not the domain's first
                    ({1: 4, 2: 6}, "mis"), ({1: 4, 2: 6}, "indel"), ({1: 3, 2: 2, 3: 5}, "indel"),   # the largest length is 2; two lengths in the last bin
                    ({0: 0, 1: 9, 2: 4, 3: 0, 4: 1, 30: 0}, "mis")):                          # zero rows, as hist() writes them
        want, n = reference_cdf(hist, e)
        got, m = characterize.empirical_cdf(hist, e)
        assert np.array_equal(got, want) and n == m, (hist, e)
    w, _ = characterize.empirical_cdf({3: 5, 4: 3, 7: 2}, "indel")
    assert len(w) == 6 and w[-1] != 1.0                      # bins of width 4 / 6: density=True divides by it, the "CDF" ends at 1.5
    assert list(characterize.empirical_cdf({1: 4, 2: 6}, "mis")[0]) == [1.0]
    for hist, e in (({1: 5}, "mis"), ({1: 5}, "indel"), ({0: 0, 1: 5, 2: 0}, "mis")):
        with pytest.raises(ValueError):
            characterize.empirical_cdf(hist, e)
    with pytest.raises(ValueError):
        characterize.empirical_cdf({}, "mis")


def test_fit_starts_are_the_reference_grids():
    m, i = characterize.fit_starts("mis"), characterize.fit_starts("indel")
    assert m.shape == (512, 3) and i.shape == (9216, 4)
    a8, a12 = np.arange(0.1, 0.9, 0.1), np.arange(0.1, 1.3, 0.1)
    assert np.array_equal(m[1], [a8[0], a8[0], a8[1]]) and np.array_equal(m[-1], [a8[-1]] * 3)
    # built as (l, p, k, w): the second entry runs to 1.2, the third to 0.8 — and ins_ll reads them as (l, k, p, w)
    assert np.array_equal(i[8 * 8 * 11 + 8 * 3 + 2], [a12[0], a12[11], a8[3], a8[2]])
    assert i[:, 1].max() == a12[-1] and i[:, 2].max() == a8[-1]


# ---- the objective alone ------------------------------------------------------------------------------------------------------------------
def test_objective_against_the_reference(fx, host):
    n_nan = n = 0
    for ent in fx["objective"]:
        e = "mis" if ent["type"] == "mis" else "indel"
        got = characterize.mixture_fit(host, e, ML.objective_cdf(fx, ent), ent["points"], evaluate=True)
        want = np.array(ent["values"])
        assert np.array_equal(np.isnan(got["fun"]), np.isnan(want)), (ent["type"], ent["set"])
        ok = ~np.isnan(want)
        worst = float(np.max(np.abs(got["fun"][ok] - want[ok])))
        print("%s on (%s): %d points, %d NaN, largest difference %.3g" % (ent["type"], ent["set"], len(want), int((~ok).sum()), worst))
        assert worst <= 1e-12, (ent["type"], ent["set"], worst)
        assert np.array_equal(ML.bits(got["fun"]), ML.bits(got["residual"])) and (got["nfev"] == 1).all() and (got["nit"] == 0).all()
        n_nan += int((~ok).sum())
        n += len(want)
    assert n == 600 and 0.15 * n < n_nan < 0.35 * n           # about a quarter of the points are invalid


# ---- the search ---------------------------------------------------------------------------------------------------------------------------
def agreement(got, want):
    both_nan = np.isnan(got) & np.isnan(want)
    with np.errstate(invalid="ignore"):
        return both_nan | (np.abs(got - want) <= 1e-9 * np.abs(want))


def test_search_against_the_reference_per_start(fx, host):
    """a start agrees when its residual is within relative 1e-9 of the reference's; at most 5 % of a grid may disagree.
    Observed with scipy 1.15.3 / numpy 2.2.6: 0 of 512, 0 of 9 216, 0 of 9 216 on (a) and 0 of 16, 0 of 64 on (b)."""
    fits = ML.host_fits(fx)
    for name, e, cdf, starts, ref_x, ref_res, _ in ML.fixture_sets(fx):
        ok = agreement(fits[name]["residual"], ref_res)
        bad = int((~ok).sum())
        print("%s: %d of %d starts disagree" % (name, bad, len(ok)))
        assert bad <= 0.05 * len(ok), "%s: %d of %d starts disagree with the reference" % (name, bad, len(ok))
        # where the residual agrees the point does too (the search ended in the same place)
        rel = np.abs(fits[name]["x"][ok] - ref_x[ok]) <= 1e-6 * np.maximum(np.abs(ref_x[ok]), 1e-3)
        assert rel.all(), name


def test_stopping_paths_of_the_fixture(fx, host):
    sets = {s[0]: s for s in ML.fixture_sets(fx)}
    _, e, cdf, _, _, _, _ = sets["a/mis"]
    # (on this fixture's histogram the grid's start (0.8, 0.8, 0.8) converges after 253 evaluations; its neighbour (0.8, 0.8, 0.7) does not)
    r = characterize.mixture_fit(host, "mis", cdf, characterize.fit_starts("mis")[[ML.MAXFEV_START]])
    assert int(r["nfev"][0]) == 600 and int(r["status"][0]) == 1 and not np.isnan(r["fun"][0])
    r = characterize.mixture_fit(host, "indel", sets["a/ins"][2], [[0.5, 0.5, 1.2, 0.5]])          # p > 1: NaN from the first evaluation on
    assert np.isnan(r["fun"][0]) and np.isnan(r["residual"][0]) and int(r["status"][0]) == 1 and int(r["nfev"][0]) == 800


def test_selection_file_and_load(fx, host, tmp_path):
    fits = ML.host_fits(fx)
    sets = {s[0]: s for s in ML.fixture_sets(fx)}
    rows = {}
    for line in fx["a"]["model_profile"].splitlines()[1:]:
        f = line.split("\t")
        rows[f[0]] = f[1:]
    for t, label in (("mis", "mismatch"), ("ins", "insertion"), ("del", "deletion")):
        name, e, _, _, ref_x, ref_res, index = sets["a/" + t]
        assert len(index) == len(characterize.fit_starts(e)), "the grid is stored thinned: selection needs every start"
        mine = characterize.select_fit(e, fits[name]["x"], fits[name]["residual"])
        ref = characterize.select_fit(e, ref_x, ref_res)
        assert mine == ref, (t, mine, ref, fits[name]["residual"][mine], ref_res[ref])
        assert np.allclose(fits[name]["x"][mine], ref_x[ref], rtol=1e-9, atol=0)
        # the reference's own file came from the same start
        want = [float(v) for v in rows[label]]
        want = want[:1] + want[2:] if t == "mis" else want
        assert np.allclose(ref_x[ref], want, rtol=1e-9, atol=0)
    # end to end: the .hist files as hist() writes them -> the file
    prefix = str(tmp_path / "training")
    for f in os.listdir(os.path.join(ROOT, "tests", "golden", "model_small")):
        shutil.copy(os.path.join(ROOT, "tests", "golden", "model_small", f), str(tmp_path / f))
    for t, _, suffix in characterize.MIXFIT_TYPES:
        h = as_hist(fx["a"]["hist"][t])
        with open(prefix + suffix, "w") as f:
            f.write("number of bases\tX:\n" + "".join("%d\t%d\n" % (k, h.get(k, 0)) for k in range(max(30, max(h) + 1))))
    fit = characterize.model_fitting(prefix, host)
    text = open(prefix + "_model_profile").read()
    assert text == characterize.format_model_profile(fit)
    got_lines, want_lines = text.splitlines(), fx["a"]["model_profile"].splitlines()
    assert got_lines[0] == want_lines[0] == "Type\tlambda\tk\tprob\tweight" and len(got_lines) == len(want_lines) == 4
    for g, w in zip(got_lines[1:], want_lines[1:]):
        g, w = g.split("\t"), w.split("\t")
        assert g[0] == w[0] and len(g) == len(w) == 5
        assert np.allclose([float(v) for v in g[1:]], [float(v) for v in w[1:]], rtol=1e-9, atol=0)
    assert got_lines[1].split("\t")[2] == "0"                 # the literal 0 of the mismatch row
    for t in ("mis", "ins", "del"):
        assert fit[t]["n_obs"] == 20000 and fit[t]["precision"] == 1.36 / math.sqrt(20000)
        assert fit[t]["warning"] == (fit[t]["residual"] > fit[t]["precision"]) and not fit[t]["warning"]
    m = model.load_model(prefix, chimeric=True, fastq=True)
    assert m.error_par["mis"] == [float(v) for v in got_lines[1].split("\t")[1:]]
    assert m.error_par["ins"] == fit["ins"]["params"] and m.error_par["del"] == fit["del"]["params"]


def test_selection_rules():
    x = np.array([[0.5, 0.5, 0.5], [0.5, 1.0, 0.5], [0.5, 0.5, 0.5], [-0.1, 0.5, 0.5], [0.5, 0.5, 0.5], [0.4, 0.4, 0.4]])
    res = np.array([0.3, 0.1, 0.2, 0.05, 0.2, np.nan])
    assert characterize.select_fit("mis", x, res) == 2          # p = 1 and l < 0 are invalid (F:131), the earlier of the tie wins, NaN never
    xi = np.array([[0.5, 2.0, 0.5, 0.5], [0.5, 0.5, 1.0, 0.5], [0.5, 0.5, 0.5, 1.0]])
    assert characterize.select_fit("indel", xi, np.array([0.3, 0.1, 0.1])) == 0     # k may pass 1 (F:164); p and w may not reach it
    assert characterize.select_fit("indel", xi[1:], np.array([0.1, 0.1])) is None


# ---- the search skeleton against scipy ------------------------------------------------------------------------------------------------------
HAND_A, HAND_B = [0.3, -1.25, 2.0, 0.75], [1.0, 3.5, 0.5, 10.0]        # tests/mixfit_host.cpp: HandQuadratic, HandBox


def quadratic(x):
    acc = 0.0
    for c in range(len(x)):
        d = float(x[c]) - HAND_A[c]
        acc = acc + (HAND_B[c] * d) * d
    return acc


def box(x):
    for c in range(len(x)):
        d = float(x[c]) - HAND_A[c]
        if d > 1.5 or d < -1.5:
            return float("nan")
    return quadratic(x)


def steps(x):
    return math.floor(quadratic(x) * 4.0) / 4.0


def slope(x):
    a, t = float(x[0]), -2e-5
    g = -1000.0 * a if a < t else -1000.0 * t - 0.5 * (a - t)
    return (g - 0.01 * float(x[1])) - 0.001 * float(x[2])


def cliff(height):
    return lambda x: height if float(x[0]) > 1.02e-3 else 0.0


HAND = (quadratic, box, steps, slope, cliff(1e-4), cliff(1.0000000000000002e-4))      # tests/mixfit_host.cpp: mixfit_host_hand's `which`


def against_scipy(host, which, x0, maxiter=None, maxfev=None):
    from scipy.optimize import minimize
    n = len(x0)
    opt = {k: v for k, v in (("maxiter", maxiter), ("maxfev", maxfev)) if v is not None}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        r = minimize(HAND[which], np.array(x0, dtype=np.float64), method="Nelder-Mead", options=opt)
    big = 0xffffffff                                          # scipy: a limit that is not given is infinite once the other one is
    h = host.hand(which, x0, (maxiter or big) if opt else 200 * n, (maxfev or big) if opt else 200 * n)
    what = (which, x0, opt)
    assert np.array_equal(ML.bits(r.x), ML.bits(list(h.x)[:n])), what
    assert (r.nfev, r.nit, r.status) == (h.nfev, h.nit, h.status), (what, r.nfev, h.nfev, r.nit, h.nit, r.status, h.status)
    assert (np.isnan(r.fun) and np.isnan(h.fun)) or r.fun == h.fun, what
    if maxfev is None or maxfev > n:                          # (below that the first simplex is not evaluated in full: its best may be an `inf` never replaced)
        assert (np.isnan(h.residual) and np.isnan(HAND[which](r.x))) or h.residual == HAND[which](r.x), what
    return r


def test_skeleton_equals_scipy(host):
    for x0 in ([1.0, 1.0, 1.0], [0.0, -1.0, 2.5], [1.0, 0.0, 1.0, 0.0], [0.5, -2.0, 3.0, 1.0], [0.0, 0.0, 0.0, 0.0]):      # zero coordinates too
        assert against_scipy(host, 0, x0).status == 0
        against_scipy(host, 1, x0)
    r = against_scipy(host, 1, [1.0, 1.0, 1.0])               # a NaN vertex stays in the simplex: no convergence, fun is NaN
    assert r.status == 1 and r.nfev == 600 and np.isnan(r.fun)
    for x0 in ([1.7, -1.0, 2.0], [1.75, -2.7, 3.4, 2.2], [-1.1, 0.2, 0.6, -0.7]):      # starts on the edge of the box
        against_scipy(host, 1, x0)


def test_skeleton_on_ties_equals_scipy(host):
    """a function in steps of 1/4: the reflected, expanded and contracted values TIE with the vertices, so every `<` and `<=` of the
    iteration decides (fxr < f[0], fxr < f[-2], fxr < f[-1], fxc <= fxr, fxcc < f[-1]), and so does the order of equal values"""
    ties = 0
    for x0 in ([1.0, 1.0, 1.0], [0.0, -1.0, 2.5], [2.3, 0.75, 2.0], [1.0, 0.0, 1.0, 0.0], [0.5, -2.0, 3.0, 1.0], [0.0, 0.0, 0.0, 0.0], [0.3, -1.25, 2.0, 4.75]):
        for maxiter in (None, 1, 2, 3, 5, 8, 13, 21, 34):
            r = against_scipy(host, 2, x0, maxiter=maxiter)
            ties += len(set(r.final_simplex[1].tolist())) < len(x0) + 1
    assert ties >= 10


def test_stop_test_at_equality_equals_scipy(host):
    """scipy stops when the largest coordinate difference AND the largest value difference to the best vertex are `<= 1e-4`
    (xatol, fatol); both are met here with EQUALITY, which no search of the fixture does.
    Values: a cliff of exactly the double 1e-4 under one vertex of the first simplex (whose coordinate steps are 5e-5): the search
    stops before its first iteration; with a cliff one ulp higher it goes on.
    Coordinates: a difference of two doubles is the double 1e-4 (an odd multiple of 2^-66) only where one of them lies below 2^-13, so
    the first simplex (steps of 0.05 x, or 0.00025) cannot tie.  `slope` makes a simplex that starts at -4.76e-5 GROW by expansions —
    steep below -2e-5, where the values differ by far more than 1e-4, gentle above — and the start is the double at which its size,
    once every vertex is on the gentle part, is 1e-4 to the bit (found by a scan over neighbouring doubles under scipy 1.15.3); the
    next double up makes it larger and the search runs on."""
    r = against_scipy(host, 4, [1e-3, 1e-3, 1e-3])
    assert (r.nfev, r.nit, r.status) == (4, 1, 0) and sorted(r.final_simplex[1].tolist()) == [0.0, 0.0, 0.0, 1e-4]
    r = against_scipy(host, 5, [1e-3, 1e-3, 1e-3])
    assert r.nfev > 4 and r.nit > 1
    tie = float.fromhex("-0x1.8f752047c70c1p-15")
    r = against_scipy(host, 3, [tie, 1e-6, 1e-6])
    sim, fsim = r.final_simplex
    assert (r.nfev, r.nit, r.status) == (21, 10, 0)
    assert float(np.max(np.abs(sim[1:] - sim[0]))) == 1e-4 and float(np.max(np.abs(fsim[0] - fsim[1:]))) < 6e-5      # the x test decides, with equality
    r = against_scipy(host, 3, [float(np.nextafter(tie, 0.0)), 1e-6, 1e-6])
    assert r.nit > 10 and r.status == 1                        # (nothing holds it once it is past: it runs down the slope to maxfev)
    r = against_scipy(host, 3, [float(np.nextafter(tie, -1.0)), 1e-6, 1e-6])
    assert (r.nfev, r.nit, r.status) == (21, 10, 0) and float(np.max(np.abs(r.final_simplex[0][1:] - r.final_simplex[0][0]))) < 1e-4


def test_skeleton_limits_equal_scipy(host):
    for x0 in ([1.0, 1.0, 1.0], [0.5, -2.0, 3.0, 1.0]):
        n = len(x0)
        for which in (0, 1):
            for maxfev in range(1, n + 40):                   # the first simplex, then every place an evaluation can be refused: reflection, expansion, both
                r = against_scipy(host, which, x0, maxfev=maxfev)      # contractions, and each vertex of a shrink
                assert r.status == 1 and r.nfev == maxfev
            for maxiter in (1, 2, 3, 10, 37):
                r = against_scipy(host, which, x0, maxiter=maxiter)
                assert r.status == 2 and r.nit == maxiter
            r = against_scipy(host, which, x0, maxiter=30, maxfev=45)
            assert r.status in (1, 2)


def test_argsort_order_is_numpys_recorded_one(fx, host):
    """MfSimplex::sort against np.argsort as recorded where the fixture was made: every pattern of 4 and 5 values over three levels and NaN"""
    n_ties = 0
    for values, order in fx["argsort"]:
        assert host.argsort(values) == order, values
        n_ties += order != [int(i) for i in np.argsort(np.array(values), kind="stable")]
    assert len(fx["argsort"]) == 4 ** 4 + 4 ** 5 and n_ties > 0      # (numpy's order is not the stable one)


# ---- the sanitizer run and the ABI ------------------------------------------------------------------------------------------------------------
def test_standalone_program_under_asan_ubsan(fx):
    """the host build as a program of its own (its main: tests/mixfit_host.cpp), exact-size heap buffers, 32 starts per type"""
    exe = ML.compile_host("mixfit_asan", ["-DMIXFIT_MAIN", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    for name, e, cdf, starts, _, _, _ in ML.fixture_sets(fx):
        pick = starts[np.linspace(0, len(starts) - 1, min(32, len(starts))).round().astype(int)]
        text = "%d %d %d\n%s\n%s\n" % (0 if e == "mis" else 1, len(cdf), len(pick), " ".join(repr(float(v)) for v in cdf),
                                      " ".join(repr(float(v)) for v in pick.ravel()))
        p = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert p.returncode == 0 and p.stdout.startswith("rc 0 ") and not p.stderr, (name, p.stdout, p.stderr[-2000:])


def test_struct_layout_export_and_argument_errors(host):
    src = r'''#include <stdio.h>
#include <stddef.h>
#include "nanosim_amd.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(ns_mixfit_fit), offsetof(ns_mixfit_fit, fun), offsetof(ns_mixfit_fit, residual),
         offsetof(ns_mixfit_fit, nfev), offsetof(ns_mixfit_fit, nit), offsetof(ns_mixfit_fit, status), offsetof(ns_mixfit_fit, reserved));
  printf("%zu %zu %d %d %d %d\n", sizeof(ns_mixfit_result), offsetof(ns_mixfit_result, ms_kernel), NS_MIXFIT_MISMATCH, NS_MIXFIT_INDEL,
         NS_MIXFIT_FIT, NS_MIXFIT_EVALUATE);
  return 0; }'''
    os.makedirs(ML.TMP, exist_ok=True)
    c = os.path.join(ML.TMP, "mixfit_layout.c")
    with open(c, "w") as f:
        f.write(src)
    exe = os.path.join(ML.TMP, "mixfit_layout")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, c])
    a, b = subprocess.check_output([exe], text=True).strip().split("\n")
    F, R = characterize.NsMixfitFit, characterize.NsMixfitResult
    assert [int(v) for v in a.split()] == [C.sizeof(F), F.fun.offset, F.residual.offset, F.nfev.offset, F.nit.offset, F.status.offset, F.reserved.offset]
    assert C.sizeof(F) == characterize.MIXFIT_DTYPE.itemsize == 64
    assert [int(v) for v in b.split()] == [C.sizeof(R), R.ms_kernel.offset, characterize.MIXFIT_MISMATCH, characterize.MIXFIT_INDEL,
                                           characterize.MIXFIT_FIT, characterize.MIXFIT_EVALUATE]
    assert "ns_mixture_fit" in engine.EXPORTS
    with open(os.path.join(ROOT, "include", "nanosim_amd.h")) as f:
        assert "#define NS_ABI_VERSION 7u" in f.read()        # an added function, no ABI bump
    cdf, x = np.array([0.5, 1.0]), np.array([0.5, 0.5, 0.5, 0.5])
    fits = np.zeros(1, dtype=characterize.MIXFIT_DTYPE)
    r = R()
    r.fits = fits.ctypes.data
    call = host.L.ns_mixture_fit
    assert call(None, 0, cdf.ctypes.data, 2, x.ctypes.data, 1, 0, C.byref(r)) == 0
    for args in ((0, None, 2, x.ctypes.data, 1, 0), (0, cdf.ctypes.data, 2, None, 1, 0), (0, cdf.ctypes.data, 0, x.ctypes.data, 1, 0),
                 (0, cdf.ctypes.data, 2, x.ctypes.data, 0, 0), (2, cdf.ctypes.data, 2, x.ctypes.data, 1, 0), (0, cdf.ctypes.data, 2, x.ctypes.data, 1, 2),
                 (-1, cdf.ctypes.data, 2, x.ctypes.data, 1, 0), (0, cdf.ctypes.data, 65537, x.ctypes.data, 1, 0)):
        assert call(None, *args, C.byref(r)) == engine.NS_EINVAL, args
    assert call(None, 0, cdf.ctypes.data, 2, x.ctypes.data, 1, 0, None) == engine.NS_EINVAL
