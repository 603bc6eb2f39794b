"""The table look-ups of the event chains, evaluated draw by draw AT their thresholds: ecdf_lookup_gv on the first-match column and on every
full match-length column, next_match_gv (ecdf_lookup_pre on the hot prefix in the LDS part, pm_lut, pm_bin, the bin search behind a previous
match >= 256), ecdf_lookup_g<double>, run_length_r, run_length_t and trans_pick_u on the packed rows (nanosim_amd/csrc/ns_chain.h,
ns_device.h), on the image ns_pack_chain_tables makes (ns_pack.h).  tests/lookup_probe.hip compiles them for the host and for gfx950; the
reference is the oracle's fp64 arithmetic on p = u32_to_p(u) (oracle/ns_oracle.c: nso_ecdf_lookup, the column choice of S:1891-1893,
run_length, trans_pick — the calls nso_error_list makes, over arrays).

The chain tests reach these look-ups through Philox draws, which land on one given edge about once in 2^32 draws; tests/test_math_probe.py
proves `p > hi <=> u >= ns_thr_gt(hi)` for the thresholds alone.  Here the draws are built FROM the packed words: thr - 1, thr, thr + 1 of
every segment, of every step of a narrow segment, of every guide cell, of the 65 536-cell guide's cells that hold an edge (every cell on
the small and the hand model), the last draw of every prefix and the first behind it, 0 and 0xffffffff, and random draws.  Previous
matches: 0, 1, 2, every bin edge -1 / +0 / +1, 255, 256, 257, the largest value a column returns, 2^31 - 1.  Run lengths: every CDF
threshold -1 / +0 / +1, every draw of l leading ones followed by zeros and the draw below it, the mixture weight's threshold -1 / +0 / +1.

What is asserted: host build == oracle on every point (CPU), gfx950 == host == oracle (the gpu half); the guides, thresholds and prefix
lengths in the packed words equal their definitions in ns_pack.h's comments, computed here from the fp64 tables (a guide that starts a
search one segment early or late gives the same answers, so only this check sees `<` against `<=` in the packer's guide loops); the hand
model's words hold every branch of the packer the synthetic models leave out (see hand_model).
ecdf_lookup_g<uint32_t> is instantiated nowhere in the engine and is not probed.  trans_pick_u: tests/test_math_probe.py covers it on
rows built by the test; here it runs on the rows as ns_pack.h packed them."""
import copy
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from nanosim_amd import model as M
from nanosim_amd import synth
from tests import oracle_lib as O
from tests.test_chain_guide import BENCH_SEED, _specs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not found")

LP_GV, LP_NEXT, LP_G64, LP_RUN_R, LP_RUN_T, LP_TRANS = range(6)
OP_NAMES = ("ecdf_lookup_gv", "next_match_gv", "ecdf_lookup_g<double>", "run_length_r", "run_length_t", "trans_pick_u")
THR_MASK, GV_UNIT, GV_NARROW = (1 << 33) - 1, 1 << 33, 1 << 34
U32_MAX = 0xffffffff
GROUPS = dict(small_and_hand=("small", "hand", "frac"), synthetic=("big", "long", "dense"), million=("bench", "trained", "octaves"))


class ChainTab(C.Structure):          # ns_device.h
    _fields_ = [(k, C.c_uint32) for k in ("n_words", "trans", "mix_w", "mix_rec", "fm_hi", "fm_vhi", "fm_n", "fm_guide", "mm_gv", "pm_lut", "sub2",
                                           "pm_bin", "n_words_lds", "fm_gv", "mm_gv_full", "pm_full", "sub2_full", "mm_g16", "int_image", "tail_bits",
                                           "n_words_mix", "mm_nbins", "mm_bin", "mm_bin_lut", "mm_seg_off", "mm_hi", "mm_vhi", "mm_vlo0", "mm_guide")] + \
               [("fm_vlo0", C.c_double)]


def build_probe(tmp, gpu, extra=()):
    src = os.path.join(ROOT, "tests", "lookup_probe.hip")
    hipcc = HIPCC if os.path.exists(HIPCC) else "hipcc"
    if gpu:
        import __graft_entry__ as G
        out = os.path.join(tmp, "lookup_probe_gfx950.so")
        cmd = [hipcc] + G.HIP_FLAGS + list(extra) + ["-o", out, src]
    else:
        out = os.path.join(tmp, "lookup_probe_host.so")
        cmd = [hipcc, "--cuda-host-only", "-x", "hip", "-O2", "-std=c++17", "-ffp-contract=off", "-DNS_HOST_TEST", *extra, "-shared", "-fPIC", "-o", out, src]
    subprocess.check_call(cmd, cwd=ROOT)
    L = C.CDLL(out)
    L.lp_gpu.restype = C.c_int
    L.lp_cells.restype = C.c_uint32; L.lp_ct_size.restype = C.c_uint32
    L.lp_cell_start.restype = C.c_uint32; L.lp_cell_start.argtypes = [C.c_uint32]
    L.lp_pack.restype = C.c_void_p; L.lp_pack.argtypes = [C.POINTER(M.NsModelTables), C.c_uint32]
    L.lp_free.restype = None; L.lp_free.argtypes = [C.c_void_p]
    L.lp_whole.restype = C.c_int; L.lp_whole.argtypes = [C.c_void_p]
    L.lp_ct.restype = None; L.lp_ct.argtypes = [C.c_void_p, C.c_void_p]
    L.lp_blob.restype = C.POINTER(C.c_uint64); L.lp_blob.argtypes = [C.c_void_p]
    L.lp_eval.restype = C.c_int; L.lp_eval.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_uint64]
    assert L.lp_gpu() == (1 if gpu else 0) and L.lp_ct_size() == C.sizeof(ChainTab)
    return L


def _oracle():
    L = O.lib()
    if not getattr(L, "_lookup_batches", False):
        L.nso_ecdf_lookup_batch.restype = None
        L.nso_ecdf_lookup_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_double, C.c_void_p, C.c_void_p, C.c_uint64]
        for f in (L.nso_next_match_batch, L.nso_trans_pick_batch):
            f.restype = None; f.argtypes = [C.POINTER(M.NsModelTables), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
        L.nso_run_length_batch.restype = None
        L.nso_run_length_batch.argtypes = [C.POINTER(M.NsModelTables)] + [C.c_void_p] * 4 + [C.c_uint64]
        L._lookup_batches = True
    return L


# ---- the arithmetic of the header comments, restated ----------------------------------------------------------------------------------
def u32_to_p(u):
    return (np.asarray(u, dtype=np.float64) + 0.5) * 2.0 ** -32          # exact: u + 0.5 has 33 significant bits


def thr_gt(t):
    """ns_thr_gt: p > t <=> u >= floor(t 2^32 - 0.5) + 1, in [0, 2^32]"""
    t = np.asarray(t, dtype=np.float64)
    y = np.floor(t * 4294967296.0 - 0.5) + 1.0
    return np.where(t < 0.0, 0.0, np.where(t >= 1.0, 4294967296.0, np.maximum(y, 0.0))).astype(np.uint64)


def thr_lt(t):
    """ns_thr_lt: p < t <=> u < ceil(t 2^32 - 0.5)"""
    t = np.asarray(t, dtype=np.float64)
    y = np.ceil(t * 4294967296.0 - 0.5)
    return np.where(~(t > 0.0), 0.0, np.where(t >= 1.0, 4294967296.0, np.maximum(y, 0.0))).astype(np.uint64)


def leading_ones_start(l):
    """the smallest draw with l leading one bits: l ones followed by zeros"""
    return 0 if l == 0 else (U32_MAX << (32 - l)) & U32_MAX


class Packed:
    """a model packed by the probe library: the ChainTab, a copy of the blob, and views of its tables"""
    def __init__(self, L, mdl, force_tail_bits=0):
        self.L, self.mdl = L, mdl
        self.t = mdl.to_c()
        self.keep = mdl._keep                                    # (the arrays the C view points into: to_c starts a new list on every call)
        self.h = L.lp_pack(C.byref(self.t), force_tail_bits)
        assert self.h
        self.ct = ChainTab()
        L.lp_ct(self.h, C.addressof(self.ct))
        self.blob = np.ctypeslib.as_array(L.lp_blob(self.h), (self.ct.n_words,)).copy()
        self.whole = bool(L.lp_whole(self.h))
        self.cols = [mdl.first_match] + list(mdl.match_markov)   # column -1 is cols[0]
        self.seg_off = np.concatenate([[0], np.cumsum([len(c.hi) for c in mdl.match_markov])]).astype(np.int64)
        self.cell_start = np.array([L.lp_cell_start(c) for c in range(L.lp_cells())], dtype=np.int64)

    def close(self):
        if self.h:
            self.L.lp_free(self.h)
            self.h = None

    def column(self, col):
        return self.cols[col + 1]

    def words(self, col):
        """the one-word segments of the FULL column"""
        if col < 0:
            return self.blob[self.ct.fm_gv:self.ct.fm_gv + self.ct.fm_n]
        o = self.ct.mm_gv_full + int(self.seg_off[col])
        return self.blob[o:o + len(self.column(col).hi)]

    def guide(self, col):
        off = self.ct.fm_guide if col < 0 else self.ct.mm_guide
        g = self.blob[off:].view(np.uint16)
        n = len(self.cell_start)
        return g[:n] if col < 0 else g[n * col:n * (col + 1)]

    def g16(self, col):
        return self.blob[self.ct.mm_g16:].view(np.uint16)[65536 * col:65536 * (col + 1)]

    def prefix(self, col):
        w = int(self.blob[self.ct.pm_bin + col])
        assert w >> 56 == col
        o, n = w & U32_MAX, (w >> 32) & 0xffffff
        return self.blob[self.ct.mm_gv + o:self.ct.mm_gv + o + n]

    def steps(self, words, sub2_off):
        """the step thresholds of the narrow segments among `words`, [(segment, thresholds)]"""
        out = []
        for s in np.nonzero(words & np.uint64(GV_NARROW))[0]:
            i = sub2_off + (int(words[s]) >> 35)
            nt = int(self.blob[i]) >> 32
            out.append((int(s), self.blob[i + 1:i + 1 + nt]))
        return out

    def run_table(self, ty, comp):
        """(thresholds, the 33 guide bytes) of one run-length table"""
        r0, r1 = int(self.blob[self.ct.mix_rec + 2 * (2 * ty + comp)]), int(self.blob[self.ct.mix_rec + 2 * (2 * ty + comp) + 1])
        go, nn = r0 & U32_MAX, r0 >> 32
        return self.blob[go:go + nn], self.blob[r1:r1 + 5].view(np.uint8)[:33]

    def eval(self, op, a, u, u2=None):
        a = np.ascontiguousarray(a, dtype=np.int32); u = np.ascontiguousarray(u, dtype=np.uint32)
        u2 = np.zeros(len(u), dtype=np.uint32) if u2 is None else np.ascontiguousarray(u2, dtype=np.uint32)
        assert len(a) == len(u) == len(u2)
        out = np.empty(len(u), dtype=np.int32)
        rc = self.L.lp_eval(self.h, op, a.ctypes.data, u.ctypes.data, u2.ctypes.data, out.ctypes.data, len(u))
        assert rc == 0, (OP_NAMES[op], rc)
        return out


# ---- the draw grids ------------------------------------------------------------------------------------------------------------------
def _around(points, rnd, rng):
    p = np.concatenate([np.asarray(x, dtype=np.int64).ravel() for x in points])
    p = np.concatenate([p - 1, p, p + 1, [0, U32_MAX], rng.integers(0, 2 ** 32, rnd, dtype=np.int64)])
    return np.unique(np.clip(p, 0, U32_MAX)).astype(np.uint32)


def column_grid(P, col, rnd, rng, every_g16_cell=False):
    """the draws of one column: on and next to every threshold its look-ups compare with"""
    w = P.words(col)
    pts = [w & np.uint64(THR_MASK), P.cell_start]
    pts += [t for _, t in P.steps(w, P.ct.sub2_full)]
    if col >= 0:
        g = P.g16(col).astype(np.int64)
        cells = np.arange(65536) if every_g16_cell else np.unique(np.concatenate([c + np.nonzero(np.diff(g))[0] for c in (0, 1)] + [[0, 65535]]))
        pts.append(cells.astype(np.int64) << 16)
        pre = P.prefix(col)
        pts.append(pre[-1:] & np.uint64(THR_MASK))               # its - 1: the last draw of the prefix; + 0: the first behind it (its first draw is 0)
        pts += [t for _, t in P.steps(pre, P.ct.sub2)]
    return _around(pts, rnd, rng)


def prev_matches(mdl):
    v = [0, 1, 2, 255, 256, 257, 2 ** 31 - 1, int(max(float(np.max(c.vhi)) for c in mdl.match_markov))]
    for c in mdl.match_markov:
        v += [c.lo - 1, c.lo, c.lo + 1, c.hi_bin - 1, c.hi_bin, c.hi_bin + 1]
    return sorted({int(x) for x in v if 0 <= x <= 2 ** 31 - 1})


def bin_of(mdl, v):
    for b, c in enumerate(mdl.match_markov):
        if c.lo <= v < c.hi_bin:
            return b
    return len(mdl.match_markov) - 1


def workload(P, rnd=10_000, every_g16_cell=False, ops=None):
    """[(op, a, u, u2, the oracle's answers)] over the grids of every table of the packed model"""
    Lo, t, mdl = _oracle(), P.t, P.mdl
    rng = np.random.default_rng(20260926)
    nb = len(mdl.match_markov)
    grids = {col: column_grid(P, col, rnd, rng, every_g16_cell) for col in range(-1, nb)}
    jobs = []
    want = (lambda op: ops is None or op in ops)
    # ---- one column, one draw
    a = np.concatenate([np.full(len(grids[col]), col, dtype=np.int32) for col in range(-1, nb)])
    u = np.concatenate([grids[col] for col in range(-1, nb)])
    ref = np.empty(len(u), dtype=np.int64)
    k = 0
    for col in range(-1, nb):
        c, g = P.column(col), grids[col]
        hi, vhi = np.ascontiguousarray(c.hi, dtype=np.float64), np.ascontiguousarray(c.vhi, dtype=np.float64)
        r = np.empty(len(g), dtype=np.int64)
        Lo.nso_ecdf_lookup_batch(hi.ctypes.data, vhi.ctypes.data, len(hi), float(c.vlo0), g.ctypes.data, r.ctypes.data, len(g))
        ref[k:k + len(g)] = r
        k += len(g)
    if P.whole and want(LP_GV):
        jobs.append((LP_GV, a, u, None, ref))
    if want(LP_G64):
        jobs.append((LP_G64, a, u, None, ref))
    # ---- the next match behind a previous one: the draws of ITS column (fewer random ones: the prefix and full column repeat per value)
    if P.whole and want(LP_NEXT):
        pm = prev_matches(mdl)
        sub = {col: np.unique(np.concatenate([grids[col][:: max(1, len(grids[col]) // 2000)], column_grid(P, col, 0, rng)])) for col in range(nb)}
        a = np.concatenate([np.full(len(sub[bin_of(mdl, v)]), v, dtype=np.int32) for v in pm])
        u = np.concatenate([sub[bin_of(mdl, v)] for v in pm])
        ref = np.empty(len(u), dtype=np.int64)
        Lo.nso_next_match_batch(C.byref(t), a.ctypes.data, u.ctypes.data, ref.ctypes.data, len(u))
        jobs.append((LP_NEXT, a, u, None, ref))
    # ---- run lengths
    if want(LP_RUN_R) or want(LP_RUN_T):
        aa, um, ul = [], [], []
        for ty in range(3):
            pts = [P.run_table(ty, comp)[0] for comp in range(2)]
            ones = np.array([leading_ones_start(l) for l in range(33)], dtype=np.int64)
            g = _around(pts + [ones, ones - 1], rnd, rng)       # (ones - 1 with its own neighbours: the draw below, and the one below that)
            w = int(thr_lt(mdl.mix_w[ty]))
            for m in sorted({min(max(x, 0), U32_MAX) for x in (w - 1, w, w + 1, 0, U32_MAX)}):
                aa.append(np.full(len(g), ty, dtype=np.int32)); um.append(np.full(len(g), m, dtype=np.uint32)); ul.append(g)
        a, u, u2 = np.concatenate(aa), np.concatenate(um), np.concatenate(ul)
        ref = np.empty(len(u), dtype=np.int64)
        Lo.nso_run_length_batch(C.byref(t), a.ctypes.data, u.ctypes.data, u2.ctypes.data, ref.ctypes.data, len(u))
        jobs += [(op, a, u, u2, ref) for op in (LP_RUN_R, LP_RUN_T) if want(op)]
    # ---- transition rows
    if want(LP_TRANS):
        aa, uu = [], []
        for st in range(7):
            g = _around([thr_lt(np.asarray(mdl.trans[st][:2], dtype=np.float64))], rnd // 10, rng)
            aa.append(np.full(len(g), st, dtype=np.int32)); uu.append(g)
        a, u = np.concatenate(aa), np.concatenate(uu)
        ref = np.empty(len(u), dtype=np.int64)
        Lo.nso_trans_pick_batch(C.byref(t), a.ctypes.data, u.ctypes.data, ref.ctypes.data, len(u))
        jobs.append((LP_TRANS, a, u, None, ref))
    return jobs


def assert_equal(got, ref, op, a, u, u2, what):
    bad = np.nonzero(got.astype(np.int64) != np.asarray(ref, dtype=np.int64))[0]
    if len(bad):
        i = bad[0]
        raise AssertionError("%s: %s differs on %d of %d points; first: a = %d, u = %#x, u2 = %#x -> %d against %d" %
                             (what, OP_NAMES[op], len(bad), len(got), int(a[i]), int(u[i]), 0 if u2 is None else int(u2[i]), int(got[i]), int(ref[i])))


def run_against_oracle(P, jobs, what):
    """every job through the probe library of P; {op: answers}"""
    out = {}
    for op, a, u, u2, ref in jobs:
        got = P.eval(op, a, u, u2)
        assert_equal(got, ref, op, a, u, u2, what)
        out[op] = got
    return out


# ---- what ns_pack.h's comments promise of the packed words ----------------------------------------------------------------------------
def check_definitions(P, what):
    mdl, ct = P.mdl, P.ct
    nb = len(mdl.match_markov)
    assert ct.mm_nbins == nb and ct.fm_n == len(mdl.first_match.hi) and ct.int_image == int(P.whole), what
    assert np.array_equal(P.blob[ct.trans:ct.trans + 21], thr_lt(np.asarray(mdl.trans, dtype=np.float64).ravel())), what
    assert np.array_equal(P.blob[ct.mix_w:ct.mix_w + 3], thr_lt(np.asarray(mdl.mix_w, dtype=np.float64))), what
    for ty in range(3):
        for comp in range(2):
            G, g2 = P.run_table(ty, comp)
            assert np.array_equal(G, thr_gt(mdl.mix_cdf[ty][comp])), (what, ty, comp)
            # g[l] = thresholds at or below the smallest draw with l leading ones, short of the last entry, saturated at 255
            for l in range(33):
                n_le = int(np.searchsorted(G, np.uint64(leading_ones_start(l)), side="right"))
                assert g2[l] == min(255, min(n_le, len(G) - 1)), (what, ty, comp, l, int(g2[l]), n_le)
    edge = P.cell_start.astype(np.float64) * 2.0 ** -32
    for col in range(-1, nb):
        c = P.column(col)
        hi = np.asarray(c.hi, dtype=np.float64)
        w = P.words(col)
        thr = w & np.uint64(THR_MASK)
        assert np.array_equal(thr, thr_gt(hi)), (what, col)
        # g[cell] = #{s : hi[s] < the cell's smallest draw / 2^32}
        assert np.array_equal(P.guide(col), np.minimum(np.searchsorted(hi, edge, side="left"), 65535)), (what, col)
        if col < 0:
            continue
        # the 65 536-cell guide: g[i] = #{s : thr(s) <= i << 16}
        assert np.array_equal(P.g16(col), np.minimum(np.searchsorted(thr, np.arange(65536, dtype=np.uint64) << np.uint64(16), side="right"), 65535)), (what, col)
        # the prefix: the segments whose threshold is below the cut and the one that crosses it; the same thresholds and classes
        pre = P.prefix(col)
        if ct.tail_bits:
            cut = (1 << 32) - (1 << (32 - ct.tail_bits))
            r = int(np.searchsorted(thr, np.uint64(cut), side="left"))
            assert len(pre) == (r + 1 if r < len(thr) else len(thr)), (what, col, len(pre), r)
        else:
            assert len(pre) == len(thr), (what, col)
        flags = np.uint64(THR_MASK | GV_UNIT | GV_NARROW)
        assert np.array_equal(pre & flags, w[:len(pre)] & flags), (what, col)
        if P.whole:
            # a unit-wide segment's value, a narrow segment's step list: as the fp64 formula gives them at the segment's draws
            for s, steps in P.steps(w, ct.sub2_full):
                head = int(P.blob[ct.sub2_full + (int(w[s]) >> 35)])
                assert head & U32_MAX == int(c.vhi[s]) and head >> 32 == len(steps) == int(c.vhi[s] - (c.vhi[s - 1] if s else c.vlo0)), (what, col, s)
                assert (np.diff(steps.astype(np.int64)) >= 0).all(), (what, col, s)


# ---- models --------------------------------------------------------------------------------------------------------------------------
def _col(lo, hi_bin, edges, widths, vlo0=0.0):
    edges, widths = np.asarray(edges, dtype=np.float64), np.asarray(widths, dtype=np.float64)
    assert len(edges) == len(widths) and (np.diff(edges) >= 0).all()
    return M.EcdfColumn(lo=lo, hi_bin=hi_bin, hi=edges, vhi=vlo0 + np.cumsum(widths), vlo0=vlo0)


def hand_model(small_model, cell_start):
    """the small model with columns and run-length tables that reach the branches of the packer the synthetic models leave out:
      H0 widths 1 .. 16 and 40 on edges off the grid of the draws: unit-wide, narrow and wide segments; a last edge of exactly 1.0
      H1 edges exactly u32_to_p(u) (a unit-wide segment becomes NARROW with its one step at its last draw), nextafter on both sides
      H2 an edge below 2^-33 (threshold 0), two distinct edges closer than 2^-33 and a repeated edge (equal thresholds, an empty segment),
         edges exactly on the smallest draw of a guide cell and of a cell of the 65 536-cell guide
      H3 a last edge of 0.9: the clamp s >= n
      H4 one segment; H5 one segment that ends at 0.5 (previous matches 5 .. 299: the bin search behind 256 ends here)
      H6 a geometric tail: twenty segments inside the guide's last cell (the bisection between the guide's bounds)
    run-length tables: one entry; 300 entries (the guide byte saturates at 255 and the walk goes on); thresholds exactly on, and one above,
    the smallest draw of every class of leading ones; a last entry below 1 (every draw above it gives the table's length); mixture weights on a draw and next to one; a transition row on draws"""
    m = copy.deepcopy(small_model)
    nx = np.nextafter
    w17 = list(range(1, 17)) + [40]
    e17 = [(k + 1) / 17.0 * 0.999 + 1.234567e-7 for k in range(16)]
    h0 = _col(0, 1, e17 + [1.0], w17)
    on = []
    for u in (1000, (1 << 20) + 7, 1 << 31, 3 * (1 << 30) + 12345, (1 << 32) - 5000):
        p = [float(u32_to_p(u + d)) for d in (0, 100, 200, 300, 400, 500)]
        on += [(p[0], 1), (float(nx(p[1], 0.0)), 1), (float(nx(p[2], 2.0)), 1), (p[3], 3), (float(nx(p[4], 0.0)), 2), (float(nx(p[5], 2.0)), 15)]
    h1 = _col(1, 2, [e for e, _ in on] + [1.0], [w for _, w in on] + [1])
    h2e = [2.0 ** -34, 0.3, float(nx(0.3, 1.0)), 0.6, 0.6, float(cell_start[40]) * 2.0 ** -32, float(777 << 16) * 2.0 ** -32,
           float(cell_start[200]) * 2.0 ** -32, float(cell_start[len(cell_start) - 1]) * 2.0 ** -32]
    order = np.argsort(h2e, kind="stable")
    h2 = _col(2, 3, [h2e[i] for i in order] + [1.0], [0, 1, 2, 1, 3, 1, 1, 2, 1, 1])       # (a value edge of 0 is a whole number too)
    h3 = _col(3, 4, [0.9 * e for e in e17] + [0.9], w17)
    h4 = _col(4, 5, [1.0], [5])
    h5 = _col(5, 300, [0.5], [3], vlo0=1.0)
    h6 = _col(300, 400, [0.25, 0.5] + [1.0 - 2.0 ** -k for k in range(3, 31)] + [1.0], [1] * 31)
    m.match_markov = [h0, h1, h2, h3, h4, h5, h6]
    m.first_match = _col(0, 0, h1.hi, np.diff(np.concatenate([[0.0], h1.vhi])))
    ones = [leading_ones_start(l) for l in range(1, 33)]
    m.mix_cdf = [[np.array([1.0]), np.concatenate([np.linspace(0.001, 0.9, 299), [1.0]])],
                 [np.concatenate([u32_to_p(np.array(ones) - 1), [1.0]]), np.concatenate([u32_to_p(np.array(ones[:-1])), [1.0]])],
                 [np.array([0.1, 0.2, 0.3]), np.array([0.1, 0.3])]]      # (last entries below 1, all in the class of no leading one: the cap at n behind one, two and three steps)
    m.mix_w = np.array([float(u32_to_p(12345)), 0.45, float(nx(u32_to_p(3 << 30), 0.0))])
    m.trans = np.array(small_model.trans, dtype=np.float64).copy()
    m.trans[4] = [float(u32_to_p(1 << 30)), float(u32_to_p((1 << 31) + 1)), float(u32_to_p((1 << 31) + 1))]
    return m


def too_wide_model(small_model):
    """a value edge of 2^29: one more than the 29 bits a segment word has for it — no integer image either"""
    m = copy.deepcopy(small_model)
    m.match_markov[-1].vhi = np.asarray(m.match_markov[-1].vhi, dtype=np.float64).copy()
    m.match_markov[-1].vhi[-1] = 536870912.0
    return m


def frac_model(small_model):
    """a value edge that is no whole number: the integer image is not valid (whole == 0) and the engine walks the fp64 tables"""
    m = copy.deepcopy(small_model)
    m.match_markov[0].vhi = np.asarray(m.match_markov[0].vhi, dtype=np.float64).copy()
    m.match_markov[0].vhi[3] += 0.5
    return m


_MODELS = {}


def get_model(name, small_model, tmp_root, cell_start):
    if name not in _MODELS:
        if name == "small":
            _MODELS[name] = small_model
        elif name == "hand":
            _MODELS[name] = hand_model(small_model, cell_start)
        elif name == "frac":
            _MODELS[name] = frac_model(small_model)
        else:
            spec = synth.SynthModelSpec(n_train=1_000_000, seed=BENCH_SEED, ecdf_rows=400) if name == "octaves" else _specs()[name]
            prefix = os.path.join(str(tmp_root), name, "training")
            synth.write_model(prefix, spec, write_pkl=False)
            _MODELS[name] = M.load_model(prefix)
    return _MODELS[name]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_probe(str(tmp_path_factory.mktemp("lookup_probe_host")), gpu=False)


@pytest.fixture(scope="module")
def host_tail3(tmp_path_factory):
    return build_probe(str(tmp_path_factory.mktemp("lookup_probe_host3")), gpu=False, extra=("-DNS_PACK_TAIL_BITS=3",))


@pytest.fixture(scope="module")
def model_of(small_model, tmp_path_factory, host):
    tmp = tmp_path_factory.mktemp("lookup_probe_models")
    cell_start = np.array([host.lp_cell_start(c) for c in range(host.lp_cells())], dtype=np.int64)
    return lambda name: get_model(name, small_model, tmp, cell_start)


def _sizes(name):
    """(random draws, every cell of the 65 536-cell guide?): the random part shrinks with the model, the edge part never"""
    return (10_000, True) if name in ("small", "hand", "frac") else (10_000 if name in ("dense", "long") else 2_000, False)


# ---- CPU -----------------------------------------------------------------------------------------------------------------------------
def test_the_hand_model_holds_the_branches_it_is_for(host, model_of):
    P = Packed(host, model_of("hand"))
    try:
        assert P.whole and P.ct.tail_bits == 0
        w0, w1, w2, w3, w4, w6 = (P.words(c) for c in (0, 1, 2, 3, 4, 6))
        unit, narrow = np.uint64(GV_UNIT), np.uint64(GV_NARROW)
        assert ((w0 & unit) != 0).sum() == 1 and ((w0 & narrow) != 0).sum() == 14 and ((w0 & (unit | narrow)) == 0).sum() == 2      # widths 1 | 2 .. 15 | 16, 40
        assert int(w0[-1]) & THR_MASK == 1 << 32                                          # a last edge of exactly 1.0: 2^32 in the 33-bit field
        # an edge exactly u32_to_p(u) under a unit-wide segment: NARROW, one step, at the segment's last draw; its neighbours by nextafter
        # keep (below) or lose (above) that draw and are UNIT
        s1 = dict(P.steps(w1, P.ct.sub2_full))
        on_draw = [s for s, t in s1.items() if len(t) == 1 and int(t[0]) == (int(w1[s]) & THR_MASK) - 1]
        assert len(on_draw) >= 5 and ((w1 & unit) != 0).sum() >= 10
        thr2 = (w2 & np.uint64(THR_MASK)).astype(np.int64)
        assert thr2[0] == 0 and (np.diff(thr2) == 0).sum() >= 2                          # an edge below 2^-33; equal thresholds: empty segments
        assert {int(P.cell_start[40]), 777 << 16, int(P.cell_start[200]), int(P.cell_start[-1])} <= set(thr2.tolist())
        assert int(w3[-1]) & THR_MASK < (1 << 32) - (1 << 12)                            # a last edge below 1 - 2^-20
        assert len(w4) == 1 and len(P.words(5)) == 1
        assert int(P.guide(6)[-1]) + 3 <= len(w6)                                        # three or more segments behind the last cell's entry
        G, g = P.run_table(0, 0)
        assert len(G) == 1
        G, g = P.run_table(0, 1)
        assert len(G) == 300 and g.max() == 255 and int(np.searchsorted(G, np.uint64(U32_MAX), side="right")) > 257
        G, g = P.run_table(1, 0)
        assert {leading_ones_start(l) for l in range(1, 33)} <= set(G.astype(np.int64).tolist())
        G, g = P.run_table(2, 0)
        assert len(G) == 3 and int(G[-1]) < 1 << 31 and g[0] == 0 and g[32] == 2                      # every threshold below the draw: the guide stops at n - 1
        assert float(P.column(2).vhi[0]) == 0.0
    finally:
        P.close()
    W = Packed(host, too_wide_model(model_of("small")))
    try:
        assert not W.whole
    finally:
        W.close()
    F = Packed(host, model_of("frac"))
    try:
        assert not F.whole
        z = np.zeros(1, dtype=np.uint32)
        for op in (LP_GV, LP_NEXT):                                                      # the probe refuses the integer look-ups there
            assert host.lp_eval(F.h, op, np.zeros(1, dtype=np.int32).ctypes.data, z.ctypes.data, z.ctypes.data, np.zeros(1, dtype=np.int32).ctypes.data, 1) == -3
    finally:
        F.close()


@pytest.mark.parametrize("group", list(GROUPS))
def test_host_look_ups_equal_the_oracle_at_every_threshold(host, model_of, group):
    for name in GROUPS[group]:
        P = Packed(host, model_of(name))
        try:
            check_definitions(P, name)
            rnd, every = _sizes(name)
            jobs = workload(P, rnd, every)
            n = sum(len(j[2]) for j in jobs)
            print("%s: %d look-ups, whole %d, tail_bits %d, LDS part %d B" % (name, n, P.whole, P.ct.tail_bits, 8 * P.ct.n_words_lds))
            assert n > 50_000 and {j[0] for j in jobs} == ({LP_G64, LP_RUN_R, LP_RUN_T, LP_TRANS} | ({LP_GV, LP_NEXT} if P.whole else set())), name
            run_against_oracle(P, jobs, name)
        finally:
            P.close()


TAILS = (("build", 3), ("force", 8), ("force", 14))


@pytest.mark.parametrize("how,bits", TAILS)
def test_host_prefixes_of_other_lengths(host, host_tail3, model_of, how, bits):
    """-DNS_PACK_TAIL_BITS=3 and force_tail_bits 8 and 14 (NS_TAIL_BITS of the engine): the prefixes end elsewhere, next_match_gv answers the same"""
    L = host_tail3 if how == "build" else host
    for name in ("small", "hand", "big", "trained"):
        P = Packed(L, model_of(name), 0 if how == "build" else bits)
        try:
            assert P.ct.tail_bits == bits, name
            check_definitions(P, (name, how, bits))
            run_against_oracle(P, workload(P, 2_000, False, ops=(LP_NEXT,)), (name, how, bits))
        finally:
            P.close()


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu_probe(tmp_path_factory):
    return build_probe(str(tmp_path_factory.mktemp("lookup_probe_gfx950")), gpu=True)


@pytest.fixture(scope="module")
def gpu_probe_tail3(tmp_path_factory):
    return build_probe(str(tmp_path_factory.mktemp("lookup_probe_gfx950_3")), gpu=True, extra=("-DNS_PACK_TAIL_BITS=3",))


def _gpu_host_oracle(Lh, Lg, mdl, force, jobs_of, what):
    H, G = Packed(Lh, mdl, force), Packed(Lg, mdl, force)
    try:
        assert np.array_equal(H.blob, G.blob), what                                     # the packer is host code in both builds
        assert all(getattr(H.ct, k) == getattr(G.ct, k) for k, _ in ChainTab._fields_), what
        jobs = jobs_of(H)
        h = run_against_oracle(H, jobs, (what, "host"))
        g = run_against_oracle(G, jobs, (what, "gfx950"))
        for op in h:
            assert np.array_equal(h[op], g[op]), (what, OP_NAMES[op])
        return sum(len(j[2]) for j in jobs)
    finally:
        H.close(); G.close()


@pytest.mark.gpu
@pytest.mark.parametrize("group", list(GROUPS))
def test_gpu_look_ups_equal_the_host_build_and_the_oracle(host, gpu_probe, model_of, group):
    for name in GROUPS[group]:
        rnd, every = _sizes(name)
        n = _gpu_host_oracle(host, gpu_probe, model_of(name), 0, lambda P: workload(P, rnd, every), name)
        assert n > 50_000, name


@pytest.mark.gpu
def test_gpu_prefixes_of_other_lengths(host, host_tail3, gpu_probe, gpu_probe_tail3, model_of):
    for how, bits in TAILS:
        Lh, Lg = (host_tail3, gpu_probe_tail3) if how == "build" else (host, gpu_probe)
        for name in ("small", "hand", "big", "trained"):
            _gpu_host_oracle(Lh, Lg, model_of(name), 0 if how == "build" else bits, lambda P: workload(P, 2_000, False, ops=(LP_NEXT,)), (name, how, bits))
