"""The guide of the ECDF columns (guide_cell, nanosim_amd/csrc/ns_device.h; built by ns_pack.h, read by ns_chain.h): cells by the leading
one bits of the draw, NS_GUIDE_OCTAVES x 32 of them.  A guide only says where the segment search of a draw STARTS, so the events cannot
change (tests/test_chain_host.py holds every look-up path against the oracle); what this file checks is what the guide promises —
the cell function is monotone and in range, guide[cell] <= the draw's segment <= guide[cell + 1] on every packed column — and what it is
for: the share of chain_error_list's iterations that leave the straight-line path for next_match_gv (4.13 % with 256 equal cells).
The device source is compiled for the host by tests/chain_guide_host.hip with a counting macro that no other build defines."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from nanosim_amd import model as M
from nanosim_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not found")

BENCH_SEED = 20260926                      # bench.py's SEED
TRAINED_BINS = ((0, 1), (1, 2), (2, 3), (3, 5), (5, 7), (7, 10), (10, 14), (14, 19), (19, 25), (25, 33), (33, 45), (45, 60), (60, 90), (90, 150), (150, 1500))


def _specs():
    """the small model aside: the `big`, `long` and `dense` specs of tests/test_chain_host.py, the bench spec and bench.py's --trained-shape spec"""
    return dict(
        big=synth.SynthModelSpec(n_train=3000, seed=99, ecdf_rows=1500, mm_bins=TRAINED_BINS, mm_means=tuple(20.0 + 2 * i for i in range(15)),
                                 mm_zero=(0.0,) + (0.02,) * 14, fm_mean=25.0),
        long=synth.SynthModelSpec(n_train=3000, seed=11, ecdf_rows=3000, fm_mean=150.0,
                                  mm_bins=((0, 40), (40, 120), (120, 256), (256, 700), (700, 1001), (1001, 2048), (2048, 3000)),
                                  mm_means=(150.0, 200.0, 260.0, 320.0, 380.0, 430.0, 480.0), mm_zero=(0.0,) + (0.01,) * 6),
        dense=synth.SynthModelSpec(n_train=3000, seed=7, aligned_median=2500.0, mis=(3.0, 0.0, 0.3, 0.5), ins=(8.0, 0.9, 0.12, 0.5),
                                   dele=(6.0, 0.95, 0.15, 0.5), mm_means=(2.0, 2.5, 3.0, 3.0, 3.5, 3.5, 4.0, 4.0),
                                   mm_zero=(0.0, 0.3, 0.3, 0.3, 0.3, 0.3, 0.3, 0.3), fm_mean=3.0),
        bench=synth.SynthModelSpec(n_train=1_000_000, seed=BENCH_SEED),
        trained=synth.SynthModelSpec(n_train=1_000_000, seed=BENCH_SEED, ecdf_rows=1500, mm_bins=TRAINED_BINS,
                                     mm_means=(24.0, 25.0, 26.0, 27.0, 28.0, 29.0, 30.0, 31.0, 31.0, 32.0, 33.0, 34.0, 35.0, 36.0, 36.0),
                                     mm_zero=(0.0,) + (0.03,) * 14))


def build_host(tmp):
    out = os.path.join(tmp, "chain_guide_host.so")
    cmd = [HIPCC if os.path.exists(HIPCC) else "hipcc", "--cuda-host-only", "-x", "hip", "-O2", "-std=c++17", "-ffp-contract=off", "-DNS_HOST_TEST",
           "-shared", "-fPIC", "-o", out, os.path.join(ROOT, "tests", "chain_guide_host.hip")]
    subprocess.check_call(cmd, cwd=ROOT, stderr=subprocess.DEVNULL)
    L = C.CDLL(out)
    L.cg_cells.restype = C.c_uint32; L.cg_octaves.restype = C.c_uint32
    L.cg_cell.restype = None; L.cg_cell.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    L.cg_cell_start.restype = C.c_uint32; L.cg_cell_start.argtypes = [C.c_uint32]
    L.cg_pack.restype = C.c_void_p; L.cg_pack.argtypes = [C.POINTER(M.NsModelTables)]
    L.cg_free.restype = None; L.cg_free.argtypes = [C.c_void_p]
    L.cg_lds_words.restype = C.c_uint32; L.cg_lds_words.argtypes = [C.c_void_p]
    L.cg_tail_bits.restype = C.c_uint32; L.cg_tail_bits.argtypes = [C.c_void_p]
    L.cg_whole.restype = C.c_int; L.cg_whole.argtypes = [C.c_void_p]
    L.cg_bounds.restype = C.c_uint64; L.cg_bounds.argtypes = [C.c_void_p, C.POINTER(M.NsModelTables), C.c_void_p, C.c_uint32, C.c_void_p]
    L.cg_count.restype = None; L.cg_count.argtypes = [C.c_void_p, C.c_int32, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p]
    return L


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_host(str(tmp_path_factory.mktemp("chain_guide_host")))


@pytest.fixture(scope="module")
def models(tmp_path_factory, small_model):
    tmp = tmp_path_factory.mktemp("chain_guide_models")
    out = dict(small=small_model)
    for name, spec in _specs().items():
        prefix = str(tmp / name / "training")
        synth.write_model(prefix, spec, write_pkl=False)
        out[name] = M.load_model(prefix)
    return out


def _cells(L, u):
    u = np.ascontiguousarray(u, dtype=np.uint32)
    cell = np.empty(len(u), dtype=np.uint32)
    L.cg_cell(u.ctypes.data, len(u), cell.ctypes.data)
    return cell


@pytest.fixture(scope="module")
def draws(host):
    """0 and 0xffffffff, both neighbours of every octave and cell border (the smallest draw of every cell and the draw below it, and the
    draws next to those), 10^5 random draws — sorted"""
    n = host.cg_cells()
    starts = np.array([host.cg_cell_start(c) for c in range(n)], dtype=np.int64)
    border = np.concatenate([starts + d for d in (-2, -1, 0, 1)])
    border = border[(border >= 0) & (border <= 0xffffffff)]
    rnd = np.random.default_rng(20260926).integers(0, 2 ** 32, 100_000, dtype=np.int64)
    return np.unique(np.concatenate([[0, 0xffffffff], border, rnd])).astype(np.uint32), starts


def test_cell_function_is_monotone_and_in_range(host, draws):
    u, starts = draws
    n, octaves = host.cg_cells(), host.cg_octaves()
    assert n == 32 * octaves and len(u) > 100_000
    cell = _cells(host, u)
    assert cell[0] == 0 and u[0] == 0 and u[-1] == 0xffffffff and cell[-1] == n - 1
    assert (cell < n).all() and (np.diff(cell.astype(np.int64)) >= 0).all()
    # the smallest draw of cell c lies in c and the draw below it in c - 1; the starts rise strictly: every cell is reached, in order
    assert (np.diff(starts) > 0).all() and starts[0] == 0
    assert (_cells(host, starts) == np.arange(n)).all()
    assert (_cells(host, starts[1:] - 1) == np.arange(n - 1)).all()
    # octave = leading one bits, capped: the first draw of octave l is l ones followed by zeros
    for l in range(octaves):
        assert starts[32 * l] == (0xffffffff << (32 - l)) & 0xffffffff


def test_guide_bounds_the_segment_of_every_draw_on_every_column(host, models, draws):
    u, _ = draws
    for name, mdl in models.items():
        t = mdl.to_c()
        pk = host.cg_pack(C.byref(t))
        assert pk
        try:
            checked = C.c_uint64()
            bad = host.cg_bounds(pk, C.byref(t), u.ctypes.data, len(u), C.addressof(checked))
            assert checked.value == len(u) * (t.mm_nbins + 1), name      # the first-match column and every match-length column
            assert bad == 0, (name, bad, checked.value)
        finally:
            host.cg_free(pk)


def _fallback_share(L, mdl, n_pieces=300):
    t = mdl.to_c()
    pk = L.cg_pack(C.byref(t))
    assert pk
    try:
        counts = np.zeros(4, dtype=np.uint64)
        rng = np.random.default_rng(5)
        for i in range(n_pieces):
            L.cg_count(pk, int(rng.integers(2000, 30001)), BENCH_SEED, i, 0, 0, counts.ctypes.data)
        return dict(it=int(counts[0]), fallback=int(counts[1]), narrow=int(counts[2]), k1=int(counts[3]),
                    lds_bytes=8 * L.cg_lds_words(pk), tail_bits=L.cg_tail_bits(pk), whole=L.cg_whole(pk))
    finally:
        L.cg_free(pk)


def test_fallback_share_on_the_bench_model(host, models):
    """300 pieces of 2-30 kb on the bench model: at most 0.5 % of the iterations may call next_match_gv (4.13 % with the guide of 256 equal
    cells).  The LDS image stays within the 24 KB that let five 256-thread workgroups share a CU."""
    r = _fallback_share(host, models["bench"])
    share = r["fallback"] / r["it"]
    print("bench model: %d iterations, next_match_gv %d (%.4f %%), narrow in place %d, k1 %d, LDS image %d B, tail_bits %d" %
          (r["it"], r["fallback"], 100 * share, r["narrow"], r["k1"], r["lds_bytes"], r["tail_bits"]))
    assert r["whole"] and r["it"] >= 100_000
    assert r["lds_bytes"] <= 24 * 1024
    assert share <= 0.005


def test_fallback_share_on_the_trained_shape_model(host, models):
    """the same on bench.py's --trained-shape model (15 columns of ~1 000 segments, hot prefixes in LDS): at most 1 %; the image stays
    within the 44 KB of two 512-thread workgroups per CU"""
    r = _fallback_share(host, models["trained"])
    share = r["fallback"] / r["it"]
    print("trained shape: %d iterations, next_match_gv %d (%.4f %%), narrow in place %d, k1 %d, LDS image %d B, tail_bits %d" %
          (r["it"], r["fallback"], 100 * share, r["narrow"], r["k1"], r["lds_bytes"], r["tail_bits"]))
    assert r["whole"] and r["it"] >= 100_000
    assert r["lds_bytes"] <= 44 * 1024
    assert share <= 0.01
