"""GPU parity of the training side's mixture fit ("The error-length mixtures"): ns_mixture_fit (k_mixfit, csrc/ns_train.h: one
wavefront per start) against the same source compiled for the host (tests/mixfit_host.cpp) BIT FOR BIT — x, fun, residual, nfev, nit and
status of every start.  What the host build owes the reference is tests/test_mixfit.py's business.  (The file sorts behind every other
-m gpu file: this is the newest kernel of the engine — and for the same reason it runs in a CHILD pytest first, like
tests/test_gpu_zzzzzz_sam_pairs.py: a device fault or a hang there fails this file with the child's output, not the whole -m gpu run.)"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from nanosim_amd import characterize
from nanosim_amd import engine as E
from tests import mixfit_lib as ML

pytestmark = pytest.mark.gpu
ROOT = ML.ROOT


@pytest.fixture(scope="module")
def fx():
    return ML.load_fixture()


@pytest.fixture(scope="module")
def host():
    return ML.build_host()


@pytest.fixture(scope="module")
def child_ok():
    if os.environ.get("NS_MIXFIT_CHILD"):
        return
    try:
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider"], cwd=ROOT,
                           env=dict(os.environ, NS_MIXFIT_CHILD="1"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    except subprocess.TimeoutExpired as ex:
        pytest.fail("the child run of this file did not finish in 300 s:\n" + str(ex.stdout or "")[-3000:])
    if r.returncode != 0:
        pytest.fail("the child run of this file failed (exit %d):\n%s" % (r.returncode, r.stdout[-4000:]))


@pytest.fixture(scope="module")
def eng(child_ok):
    e = E.Engine(0)
    yield e
    e.close()


def same(g, h, what):
    """two results of characterize.mixture_fit: the same bits in every field"""
    for k in ("x", "fun", "residual"):
        assert np.array_equal(ML.bits(g[k]), ML.bits(h[k])), (what, k, int((ML.bits(g[k]) != ML.bits(h[k])).sum()))
    for k in ("nfev", "nit", "status"):
        assert np.array_equal(g[k], h[k]), (what, k)


def both(eng, host, error, cdf, starts, what, **kw):
    g = characterize.mixture_fit(eng, error, cdf, starts, **kw)
    same(g, characterize.mixture_fit(host, error, cdf, starts, **kw), what)
    return g


def seeded_cdf(rng, n):
    """a monotone CDF of n bins that ends at 1"""
    c = np.cumsum(rng.random(n) ** 3 + 1e-6)
    c /= c[-1]
    c[-1] = 1.0
    return c


def some_points(rng, n, dim):
    p = np.column_stack([rng.uniform(0.05, 3.0, n)] + ([rng.uniform(0.1, 2.0, n)] if dim == 4 else []) + [rng.uniform(0.01, 1.0, n), rng.uniform(0.01, 0.99, n)])
    p[0, -1] = 1.3                     # the clip bites
    p[1, 0] = -0.5                     # NaN
    p[2, dim - 2] = 1.0                # p = 1
    return p


def test_gpu_objective_fixture_points(fx, eng, host):
    n = 0
    for ent in fx["objective"]:
        e = "mis" if ent["type"] == "mis" else "indel"
        g = both(eng, host, e, ML.objective_cdf(fx, ent), ent["points"], (ent["type"], ent["set"]), evaluate=True)
        assert np.array_equal(np.isnan(g["fun"]), np.isnan(np.array(ent["values"])))
        n += len(ent["points"])
    assert n == 600


@pytest.mark.parametrize("n_bins", [1, 2, 63, 64, 65, 127, 128, 129, 1000])
def test_gpu_objective_tile_borders(eng, host, n_bins):
    rng = np.random.default_rng(1000 + n_bins)
    cdf = seeded_cdf(rng, n_bins)
    for e, dim in (("mis", 3), ("indel", 4)):
        g = both(eng, host, e, cdf, some_points(rng, 8, dim), (e, n_bins), evaluate=True)
        assert np.isnan(g["fun"][1]) and not np.isnan(np.delete(g["fun"], 1)).any()


def test_gpu_fits_every_mismatch_start(fx, eng, host):
    name, e, cdf, starts, _, _, _ = ML.fixture_sets(fx)[0]
    assert name == "a/mis" and len(starts) == 512
    g = characterize.mixture_fit(eng, e, cdf, starts)
    same(g, ML.host_fits(fx)[name], name)
    assert g["ms_kernel"] > 0 and int(g["status"][ML.MAXFEV_START]) == 1 and int(g["nfev"][ML.MAXFEV_START]) == 600


@pytest.mark.parametrize("pick", ["0-63", "0-64", "stride 37"])
def test_gpu_fits_insertion_grid_full_and_partial_workgroups(fx, eng, host, pick):
    name, e, cdf, starts, _, _, index = ML.fixture_sets(fx)[1]
    assert name == "a/ins"
    rows = {"0-63": np.arange(64), "0-64": np.arange(65), "stride 37": np.arange(0, len(starts), 37)[:250]}[pick]
    assert len(rows) == {"0-63": 64, "0-64": 65, "stride 37": 250}[pick]
    want = ML.host_fits(fx)[name]
    g = characterize.mixture_fit(eng, e, cdf, starts[rows])
    same(g, {k: want[k][rows] for k in ("x", "fun", "residual", "nfev", "nit", "status")}, pick)
    if pick == "stride 37":
        for n in (1, 3):               # one wavefront, and a workgroup that is not full
            same(characterize.mixture_fit(eng, e, cdf, starts[rows[:n]]), {k: want[k][rows[:n]] for k in ("x", "fun", "residual", "nfev", "nit", "status")}, n)


def test_gpu_fits_long_tail_sets(fx, eng, host):
    fits = ML.host_fits(fx)
    for name, e, cdf, starts, _, _, _ in ML.fixture_sets(fx)[3:]:
        assert len(cdf) in (150, 131)
        same(characterize.mixture_fit(eng, e, cdf, starts), fits[name], name)


def test_gpu_fits_1000_bins(eng, host):
    rng = np.random.default_rng(77)
    cdf = seeded_cdf(rng, 1000)
    both(eng, host, "mis", cdf, characterize.fit_starts("mis")[[0, 170, 341, 511]], "mis 1000")
    both(eng, host, "indel", cdf, characterize.fit_starts("indel")[[0, 3071, 6143, 9215]], "indel 1000")


def test_gpu_stopping_paths(fx, eng, host):
    sets = ML.fixture_sets(fx)
    g = both(eng, host, "mis", sets[0][2], characterize.fit_starts("mis")[[ML.MAXFEV_START]], "maxfev")
    assert (int(g["nfev"][0]), int(g["status"][0])) == (600, 1)
    g = both(eng, host, "indel", sets[1][2], [ML.NAN_START], "a NaN simplex")
    assert np.isnan(g["fun"][0]) and np.isnan(g["residual"][0]) and (int(g["nfev"][0]), int(g["status"][0])) == (800, 1)


def test_gpu_model_profile_end_to_end(fx, eng, host, tmp_path):
    texts = []
    for who, e in (("gpu", eng), ("host", host)):
        prefix = str(tmp_path / who)
        for t, _, suffix in characterize.MIXFIT_TYPES:
            h = {int(k): int(v) for k, v in fx["a"]["hist"][t]}
            with open(prefix + suffix, "w") as f:
                f.write("number of bases\tX:\n" + "".join("%d\t%d\n" % (k, h.get(k, 0)) for k in range(max(30, max(h) + 1))))
        fit = characterize.model_fitting(prefix, e)
        texts.append((open(prefix + "_model_profile").read(), {t: (fit[t]["start"], fit[t]["residual"], fit[t]["warning"]) for t in fit}))
    assert texts[0] == texts[1] and texts[0][0].count("\n") == 4


def test_gpu_engine_state_and_argument_errors(fx, eng, host):
    sets = ML.fixture_sets(fx)
    both(eng, host, "indel", sets[2][2], sets[2][3][:5], "small call")
    both(eng, host, "mis", sets[3][2], sets[3][3], "larger call")
    pairs = [("AAAAAACGTCGTTTTTT", "AAAAAACGTCGTTTTTT"), ("GGGGG-GACGTACCCCCCC", "GGGGGAGACGTAC-CCCCC")]
    t = characterize.count_homopolymers(eng, pairs, min_hp_len=5)
    assert t["n_hp"] > 0 and t["ms_kernel"] > 0
    both(eng, host, "indel", sets[2][2], sets[2][3][:5], "again")
    cdf, x = np.array([0.5, 1.0]), np.array([0.5, 0.5, 0.5, 0.5])
    fits = np.zeros(1, dtype=characterize.MIXFIT_DTYPE)
    r = characterize.NsMixfitResult()
    r.fits = fits.ctypes.data
    call = eng.L.ns_mixture_fit
    for args in ((0, None, 2, x.ctypes.data, 1, 0), (0, cdf.ctypes.data, 2, None, 1, 0), (0, cdf.ctypes.data, 0, x.ctypes.data, 1, 0),
                 (0, cdf.ctypes.data, 2, x.ctypes.data, 0, 0), (2, cdf.ctypes.data, 2, x.ctypes.data, 1, 0), (0, cdf.ctypes.data, 2, x.ctypes.data, 1, 2),
                 (0, cdf.ctypes.data, 65537, x.ctypes.data, 1, 0)):
        assert call(eng.ctx, *args, C.byref(r)) == E.NS_EINVAL, args
        assert b"ns_mixture_fit" in eng.L.ns_last_error(eng.ctx)
    assert call(eng.ctx, 0, cdf.ctypes.data, 2, x.ctypes.data, 1, 0, None) == E.NS_EINVAL
    r.fits = None
    assert call(eng.ctx, 0, cdf.ctypes.data, 2, x.ctypes.data, 1, 0, C.byref(r)) == E.NS_EINVAL
    assert call(None, 0, cdf.ctypes.data, 2, x.ctypes.data, 1, 0, C.byref(r)) == E.NS_EINVAL
    r.fits = fits.ctypes.data
    assert call(eng.ctx, 0, cdf.ctypes.data, 2, x.ctypes.data, 1, 0, C.byref(r)) == 0 and fits["nfev"][0] > 0
