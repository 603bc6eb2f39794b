"""The engine's base-quality look-ups, evaluated directly over every 16-bit draw: qual_value (binary search), qual_value_lut (bucket table +
carry, flagged buckets walked), qual_lookup16 (two draws per dword, the ballot redo through qual_value) and the bucket-table builder of
ns_load_model (ns_build_qual_lut).  tests/qual_probe.hip compiles them for the host and for gfx950 (qual_lookup16 on one wavefront with its
tables in LDS, as k_qualities runs it); the exact count q = #{j < 127 : h >= thr[j]} (np.searchsorted) is the reference.

The Python loader snaps its tables so that no bucket holds two thresholds (model.snap_quality_thresholds): the whole-batch parity tests
never set a bucket's walk flag.  The tables here do: the raw closed-form tables, adversarial layouts (up to 127 thresholds in one bucket,
thresholds at and next to bucket edges, runs of equal thresholds, entries of 0, 65535 and 65536 or more) and the walk tables of
tests/test_gpu_qual_walk.py.

What is asserted:
  - host qual_value == host qual_value_lut == the exact count, for every table, class and h (the GPU half, marked gpu: the same for the
    gfx950 build and qual_lookup16, in waves where no lane, exactly one lane or every lane reads a flagged bucket);
  - every builder entry equals a restatement of its documented layout;
  - snap_quality_thresholds on random non-decreasing tables: monotone output, at most one threshold strictly inside any bucket, no
    threshold moved by more than 32, and a table that already has that property unchanged."""
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

LEVELS = 128                         # NS_QUAL_LEVELS: thr[0..126] are compared, thr[127] never
NCLS = 5                             # NS_Q_COUNT, in the order of NS_Q_NAMES
Q_MATCH, Q_MIS, Q_INS, Q_HT, Q_UNMAPPED = range(NCLS)
ALL_H = np.arange(1 << 16, dtype=np.uint32)


def _hipcc():
    return HIPCC if os.path.exists(HIPCC) else "hipcc"


def build_probe(tmp, gpu):
    """tests/qual_probe.hip for the host (--cuda-host-only -DNS_HOST_TEST, as tests/test_math_probe.py) or for gfx950 with the engine's
    flags (__graft_entry__.HIP_FLAGS), into tmp"""
    src = os.path.join(ROOT, "tests", "qual_probe.hip")
    if gpu:
        import __graft_entry__ as G
        out = os.path.join(tmp, "qual_probe_gfx950.so")
        cmd = [_hipcc()] + G.HIP_FLAGS + ["-o", out, src]
    else:
        out = os.path.join(tmp, "qual_probe_host.so")
        cmd = [_hipcc(), "--cuda-host-only", "-x", "hip", "-O3", "-std=c++17", "-ffp-contract=off", "-DNS_HOST_TEST", "-shared", "-fPIC",
               "-o", out, src]
    subprocess.check_call(cmd, cwd=ROOT)
    return load_probe(out, gpu)


def load_probe(path, gpu):
    L = C.CDLL(path)
    L.probe_gpu.restype = C.c_int; L.probe_gpu.argtypes = []
    L.probe_build_lut.restype = C.c_int; L.probe_build_lut.argtypes = [C.c_void_p, C.c_void_p]
    L.probe_thr_decrease.restype = C.c_uint32; L.probe_thr_decrease.argtypes = [C.c_void_p]
    L.probe_qual_value.restype = C.c_int; L.probe_qual_value.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
    L.probe_qual_value_lut.restype = C.c_int
    L.probe_qual_value_lut.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
    if gpu:
        L.probe_lookup16.restype = C.c_int
        L.probe_lookup16.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    assert L.probe_gpu() == (1 if gpu else 0)
    return L


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_probe(str(tmp_path_factory.mktemp("qual_probe_host")), gpu=False)


# ---- references ------------------------------------------------------------------------------------------------------------------
def exact(thr, h=ALL_H):
    """q = #{j < 127 : h >= thr[j]} for a non-decreasing thr"""
    return np.searchsorted(np.asarray(thr, dtype=np.int64)[:LEVELS - 1], np.asarray(h, dtype=np.int64), side="right").astype(np.uint8)


def lut_spec(thr):
    """the documented layout of a bucket entry (ns_pack.h ns_build_qual_lut, ns_device.h DevModel::qual_lut): bits 7-13 the count of
    thresholds at or below the bucket start 64 b, bits 0-6 128 minus the offset of the first threshold strictly inside the bucket (64 if
    none), bit 15 when two or more lie strictly inside"""
    t = np.asarray(thr, dtype=np.int64)[:LEVELS - 1]
    out = np.empty(1024, dtype=np.uint16)
    for b in range(1024):
        lo = 64 * b
        inside = t[(t > lo) & (t <= lo + 63)]
        sub = int(inside[0]) - lo if len(inside) else 64
        out[b] = (int(np.sum(t <= lo)) << 7) | (128 - sub) | (0x8000 if len(inside) >= 2 else 0)
    return out


def inside_counts(t):
    """the number of entries of t strictly inside each bucket (64 b, 64 b + 63]"""
    t = np.asarray(t, dtype=np.int64)
    t = t[(t > 0) & (t < 65536) & (t % 64 != 0)]
    return np.bincount(t // 64, minlength=1024)


def flagged(thr):
    """the buckets with two or more of the compared thresholds thr[0..126] strictly inside"""
    return inside_counts(np.asarray(thr)[:LEVELS - 1]) >= 2


# ---- tables ----------------------------------------------------------------------------------------------------------------------
def _small_model_quals():
    m = M.load_model(os.path.join(ROOT, "tests", "golden", "model_small", "training"), fastq=True)
    return m.quals


def model_tables():
    """{name: [5 tables in class order]}: the small model and every operating point of synth, raw (quality_thresholds) and snapped (what
    model.load_model hands the engine)"""
    sets = {}
    for src, quals in [("model_small", _small_model_quals())] + [(n, synth.operating_point_spec(n).quals) for n in synth.OPERATING_POINTS]:
        raw = [M.quality_thresholds(*quals[nm]) for nm in M.NS_Q_NAMES]
        sets[src + "/raw"] = raw
        sets[src + "/snapped"] = [M.snap_quality_thresholds(t) for t in raw]
    return sets


def _table(head, tail=65536):
    """thr[0..len(head)) = head (sorted), the rest = tail"""
    t = np.full(LEVELS, tail, dtype=np.int64)
    t[:len(head)] = np.sort(np.asarray(head, dtype=np.int64))
    return t.astype(np.uint32)


def adversarial_tables():
    """{name: table}"""
    rng = np.random.default_rng(20261016)
    out = {}
    b = 300
    for n in (2, 3, 5, 16, 63, 64, 127):                      # n thresholds strictly inside bucket b, the others spread below and above it
        offs = np.sort(np.concatenate([np.arange(1, 64), rng.integers(1, 64, 64)])[:n]) if n > 63 else np.sort(rng.choice(np.arange(1, 64), n, replace=False))
        rest = LEVELS - 1 - n
        below = np.sort(rng.integers(0, 64 * b + 1, rest // 2))
        above = np.sort(rng.integers(64 * b + 64, 65536, rest - rest // 2))
        out["inside%d" % n] = _table(np.concatenate([below, 64 * b + offs, above]))
    out["inside2_at_edges"] = _table([64 * 7 + 1, 64 * 7 + 63])
    # 64 b, 64 b + 1 and 64 b + 63 for the first, a middle and the last bucket (0, 1, 63, ..., 65472, 65473, 65535)
    edges = [64 * bb + o for bb in (0, 1, 2, 511, 512, 1022, 1023) for o in (0, 1, 63)]
    out["bucket_edges"] = _table(edges)
    out["bucket_edges_sparse"] = _table([64 * bb + o for bb, o in ((0, 1), (3, 0), (5, 63), (9, 1), (9, 63), (1023, 63))])
    out["equal_runs"] = _table([0] * 5 + [64 * 40] * 9 + [64 * 41 + 17] * 20 + [64 * 41 + 30] + [64 * 900 + 5] * 30 + [65535] * 10)
    out["thr0_zero"] = _table([0] + list(range(100, 12700, 100)))
    out["tail_65535"] = _table(list(range(500, 60000, 1000)) + [65535] * 20, tail=65535)
    out["tail_beyond"] = _table(list(range(900, 63000, 1000)), tail=0xffffffff)
    big = np.arange(LEVELS, dtype=np.int64) * 513
    big[100:] = [65536, 65537, 70000, 1 << 20, 0x7fffffff, 0xfffffffe] + [0xffffffff] * 22
    out["entries_65536_and_above"] = big.astype(np.uint32)
    out["all_zero"] = np.zeros(LEVELS, dtype=np.uint32)
    out["all_65536"] = np.full(LEVELS, 65536, dtype=np.uint32)
    out["all_65535"] = np.full(LEVELS, 65535, dtype=np.uint32)
    out["max_flagged"] = _table([64 * (16 * k + 8) + o for k in range(63) for o in (1 + k % 3, 63 - k % 4)] + [64 * 1015 + 9])
    for i in range(4):                                        # random clusters: several thresholds per bucket, runs, gaps
        c = rng.integers(0, 1024, 12)
        out["clusters%d" % i] = _table(np.clip(np.repeat(c * 64, 11)[:LEVELS - 1] + rng.integers(-40, 100, LEVELS - 1), 0, 65536))
    # the last compared entry thr[126] and the never-read thr[127] (set below it: not part of the table)
    t = np.arange(LEVELS, dtype=np.int64) * 500; t[127] = 0
    out["thr127_ignored"] = t.astype(np.uint32)
    return out


def walk_tables():
    """Five non-decreasing class tables (class order) whose flagged buckets carry 63 / 1024 of every class's mass — the most 127
    thresholds allow (a flagged bucket takes two) — and whose walk-only levels are private to one class.

    Pair k = 0..62 (thr[2 k], thr[2 k + 1]) lies strictly inside bucket 16 k + 8.  For class c = k mod 5 the pair is two distinct offsets:
    level 2 k + 1 lies between two thresholds of one bucket, so only the walk (qual_value_lut) or the redo (qual_lookup16) can emit it.
    For the other classes the pair is one threshold twice: still a flagged bucket, but level 2 k + 1 has no mass.  thr[126] = 65536: never
    reached.  The levels between pairs (even) are shared by all classes."""
    tabs = []
    for c in range(NCLS):
        t = np.full(LEVELS, 65536, dtype=np.int64)
        for k in range(63):
            lo = 64 * (16 * k + 8)
            if k % NCLS == c:
                t[2 * k], t[2 * k + 1] = lo + 1 + k % 3, lo + 63 - k % 4
            else:
                t[2 * k] = t[2 * k + 1] = lo + 32
        tabs.append(t.astype(np.uint32))
    return tabs


def walk_only_levels(c):
    """the levels only class c of walk_tables() can emit, and only through the walk"""
    return [2 * k + 1 for k in range(63) if k % NCLS == c]


def all_class_tables():
    """(name, table) for every single table checked on its own: each class of every model set, the walk tables, the adversarial ones"""
    out = []
    for name, tabs in model_tables().items():
        out += [("%s/%s" % (name, M.NS_Q_NAMES[c]), t) for c, t in enumerate(tabs)]
    out += [("walk/%s" % M.NS_Q_NAMES[c], t) for c, t in enumerate(walk_tables())]
    out += sorted(adversarial_tables().items())
    return out


def table_sets():
    """(name, [5 tables]) for qual_lookup16, which reads the tables of all classes: the model sets, the walk tables, the adversarial
    tables five at a time"""
    sets = list(model_tables().items()) + [("walk", walk_tables())]
    adv = sorted(adversarial_tables().items())
    for i in range(0, len(adv), NCLS):
        grp = adv[i:i + NCLS]
        grp += adv[:NCLS - len(grp)]
        sets.append(("adversarial:" + ",".join(n for n, _ in grp), [t for _, t in grp]))
    return sets


# ---- probe calls -------------------------------------------------------------------------------------------------------------------
def build_lut(L, thr):
    thr = np.ascontiguousarray(thr, dtype=np.uint32)
    lut = np.empty(1024, dtype=np.uint16)
    assert L.probe_build_lut(thr.ctypes.data, lut.ctypes.data) == 0
    return lut


def qual_value(L, thr, h=ALL_H):
    thr = np.ascontiguousarray(thr, dtype=np.uint32); h = np.ascontiguousarray(h, dtype=np.uint32)
    out = np.empty(len(h), dtype=np.uint8)
    assert L.probe_qual_value(thr.ctypes.data, h.ctypes.data, out.ctypes.data, len(h)) == 0
    return out


def qual_value_lut(L, thr, lut, h=ALL_H):
    thr = np.ascontiguousarray(thr, dtype=np.uint32); lut = np.ascontiguousarray(lut, dtype=np.uint16)
    h = np.ascontiguousarray(h, dtype=np.uint32)
    out = np.empty(len(h), dtype=np.uint8)
    assert L.probe_qual_value_lut(thr.ctypes.data, lut.ctypes.data, h.ctypes.data, out.ctypes.data, len(h)) == 0
    return out


def assert_same(got, exp, what):
    bad = np.nonzero(got != exp)[0]
    if len(bad):
        i = int(bad[0])
        raise AssertionError("%s: %d of %d draws differ; first h = %d: %d against %d" % (what, len(bad), len(got), i, int(got[i]), int(exp[i])))


# ---- host build (every CPU run) ----------------------------------------------------------------------------------------------------
def test_tables_reach_flagged_buckets():
    """the table sets hold what they are for: flagged buckets in every raw model class, none in the snapped ones, 63 in every walk class,
    up to 127 thresholds in one bucket"""
    for name, tabs in model_tables().items():
        for c, t in enumerate(tabs):
            assert np.all(np.diff(t.astype(np.int64)[:LEVELS - 1]) >= 0), name
            n = int(flagged(t).sum())
            assert (n == 0) if name.endswith("/snapped") else (n > 0), (name, M.NS_Q_NAMES[c], n)
    for c, t in enumerate(walk_tables()):
        assert int(flagged(t).sum()) == 63
        e = exact(t)
        for lv in range(1, 126, 2):
            assert (int(np.sum(e == lv)) > 0) == (lv in walk_only_levels(c)), (c, lv)
        assert not np.any(np.isin(e[~np.repeat(flagged(t), 64)], walk_only_levels(c)))
    adv = adversarial_tables()
    assert int(np.max(np.bincount(adv["inside127"][:LEVELS - 1].astype(np.int64) // 64))) == 127
    assert all(np.all(np.diff(t.astype(np.int64)[:LEVELS - 1]) >= 0) for t in adv.values())


def test_host_lookups_equal_exact_count(host):
    """host qual_value == host qual_value_lut (on the builder's table) == the exact count, for every table and class, all 65 536 h"""
    n = 0
    for name, thr in all_class_tables():
        ex = exact(thr)
        assert_same(qual_value(host, thr), ex, name + ": qual_value")
        lut = build_lut(host, thr)
        assert_same(qual_value_lut(host, thr, lut), ex, name + ": qual_value_lut")
        # every bucket flagged: the walk from the count at each bucket start alone gives the count
        assert_same(qual_value_lut(host, thr, lut | np.uint16(0x8000)), ex, name + ": qual_value_lut, every bucket walked")
        n += 1
    assert n >= 60


def test_builder_matches_its_layout(host):
    for name, thr in all_class_tables():
        got, exp = build_lut(host, thr), lut_spec(thr)
        bad = np.nonzero(got != exp)[0]
        assert not len(bad), "%s: bucket %d: %#06x against %#06x" % (name, int(bad[0]), int(got[bad[0]]), int(exp[bad[0]]))
        assert host.probe_thr_decrease(np.ascontiguousarray(thr, dtype=np.uint32).ctypes.data) == 0, name


def test_decreasing_tables_are_found(host):
    """ns_qual_thr_decrease (ns_load_model's check): the first level j in 1..126 with thr[j] < thr[j - 1]; thr[127] is not part of it"""
    base = (np.arange(LEVELS, dtype=np.uint32) + 1) * 400
    for j in (1, 2, 63, 64, 125, 126):
        t = base.copy(); t[j] = t[j - 1] - 1
        assert host.probe_thr_decrease(t.ctypes.data) == j
        t = base.copy(); t[j - 1] = 0xffffffff
        assert host.probe_thr_decrease(t.ctypes.data) == j
    t = base.copy(); t[127] = 0
    assert host.probe_thr_decrease(t.ctypes.data) == 0
    t = base.copy(); t[10] = t[9]; t[11] = t[9]
    assert host.probe_thr_decrease(t.ctypes.data) == 0


# ---- snap_quality_thresholds -------------------------------------------------------------------------------------------------------
def _random_monotone(rng):
    kind = rng.integers(0, 5)
    if kind == 0:                                             # uniform over the draw range
        t = rng.integers(0, 65537, LEVELS)
    elif kind == 1:                                           # clustered: a few buckets with many thresholds each
        t = np.repeat(rng.integers(0, 1024, 8) * 64, 16) + rng.integers(0, 64, LEVELS)
    elif kind == 2:                                           # a closed-form table of random parameters
        return M.quality_thresholds(float(rng.uniform(0.2, 0.8)), float(rng.integers(0, 5)), float(rng.uniform(1.5, 3.5)))
    elif kind == 3:                                           # runs of equal values and edges
        t = rng.choice(np.concatenate([[0, 1, 63, 64, 65, 65535, 65536], rng.integers(0, 65537, 8)]), LEVELS)
    else:                                                     # at most one threshold inside any bucket: nothing to move
        t = np.concatenate([rng.choice(1024, 64, replace=False) * 64 + rng.integers(1, 64, 64), rng.integers(0, 1025, 64) * 64])
    return np.sort(np.clip(t, 0, 65536)).astype(np.uint32)


def test_snap_quality_thresholds_properties():
    rng = np.random.default_rng(5150)
    unchanged = 0
    for _ in range(300):
        t = _random_monotone(rng)
        s = M.snap_quality_thresholds(t)
        assert s.dtype == np.uint32 and len(s) == len(t)
        s64, t64 = s.astype(np.int64), t.astype(np.int64)
        assert np.all(np.diff(s64) >= 0), "not monotone"
        assert int(np.max(inside_counts(s))) <= 1, "two thresholds inside one bucket"
        assert int(np.max(np.abs(s64 - t64))) <= 32, "moved by more than 32"
        # already snapped: unchanged
        assert np.array_equal(M.snap_quality_thresholds(s), s)
        if int(np.max(inside_counts(t))) <= 1:
            assert np.array_equal(s, t)
            unchanged += 1
    assert unchanged >= 20


# ---- the GPU half ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu(tmp_path_factory):
    return build_probe(str(tmp_path_factory.mktemp("qual_probe_gfx950")), gpu=True)


def lookup16_lanes(tabs, luts, rng):
    """Lanes of 16 (draw, class) for qual_lookup16, and the wave kind of each group of 64 lanes.
    'all': every (h, class) once — match, substituted and inserted mixed inside each lane, ht and unmapped lanes whole — lanes shuffled;
    then, where the tables allow, waves in which no lane ('none'), exactly one lane at one position ('one') or every lane ('every')
    reads a flagged bucket."""
    fl = [np.repeat((lut & 0x8000) != 0, 64) for lut in luts]
    mixed = rng.permutation(3 << 16)
    H = [(mixed & 0xffff).astype(np.uint32).reshape(-1, 16)]
    Cl = [(mixed >> 16).astype(np.uint8).reshape(-1, 16)]
    for c in (Q_HT, Q_UNMAPPED):
        H.append(rng.permutation(ALL_H).reshape(-1, 16)); Cl.append(np.full((4096, 16), c, dtype=np.uint8))
    H, Cl = np.concatenate(H), np.concatenate(Cl)
    o = rng.permutation(len(H))
    H, Cl = H[o], Cl[o]
    kinds = ["all"] * (len(H) // 64)
    unfl = [ALL_H[~f] for f in fl]
    fla = [ALL_H[f] for f in fl]
    ok_u = [c for c in range(NCLS) if len(unfl[c])]
    ok_f = [c for c in ok_u if len(fla[c])]
    mix_f = [c for c in (Q_MATCH, Q_MIS, Q_INS) if c in ok_f]
    if ok_f and {Q_MATCH, Q_MIS, Q_INS} <= set(ok_u):
        def lane(c=None):
            cl = rng.choice([Q_MATCH, Q_MIS, Q_INS], 16) if c is None else np.full(16, c)
            return np.array([rng.choice(unfl[x]) for x in cl], dtype=np.uint32), cl.astype(np.uint8)
        for kind in ("none", "one", "every") * 8:
            h = np.empty((64, 16), dtype=np.uint32); cl = np.empty((64, 16), dtype=np.uint8)
            whole = [c for c in (Q_HT, Q_UNMAPPED) if c in ok_u]
            for ln in range(64):
                h[ln], cl[ln] = lane(None if rng.random() < 0.75 or not whole else int(rng.choice(whole)))
            for ln in ([] if kind == "none" else [int(rng.integers(64))] if kind == "one" else range(64)):
                i = int(rng.integers(16))
                if cl[ln, 0] >= Q_HT and cl[ln, 0] not in ok_f or cl[ln, 0] < Q_HT and not mix_f:
                    h[ln], cl[ln] = lane(None if mix_f else int(rng.choice(ok_f)))
                if cl[ln, 0] < Q_HT:
                    cl[ln, i] = rng.choice(mix_f)
                h[ln, i] = rng.choice(fla[int(cl[ln, i])])
            H = np.concatenate([H, h]); Cl = np.concatenate([Cl, cl]); kinds.append(kind)
    # the wave kinds hold
    lane_fl = np.zeros(len(H), dtype=bool)
    for c in range(NCLS):
        lane_fl |= np.any((Cl == c) & fl[c][H], axis=1)
    per_wave = lane_fl.reshape(-1, 64).sum(axis=1)
    for w, kind in enumerate(kinds):
        if kind != "all":
            assert per_wave[w] == {"none": 0, "one": 1, "every": 64}[kind], (kind, per_wave[w])
    # a lane of ht or unmapped is that class throughout (the constant class words of k_qualities)
    assert np.all((Cl[:, 0] < Q_HT) == np.all(Cl < Q_HT, axis=1)) and np.all(np.all(Cl == Cl[:, :1], axis=1) | (Cl[:, 0] < Q_HT))
    return H, Cl, kinds


def lookup16(L, tabs, luts, H, Cl):
    thr = np.ascontiguousarray(np.stack(tabs), dtype=np.uint32)
    lut = np.ascontiguousarray(np.stack(luts), dtype=np.uint16)
    D = np.ascontiguousarray(H.reshape(-1, 8, 2)[:, :, 0] | (H.reshape(-1, 8, 2)[:, :, 1] << np.uint32(16)), dtype=np.uint32)
    cl = np.ascontiguousarray(Cl, dtype=np.uint8)
    out = np.empty((len(H), 16), dtype=np.uint8)
    assert len(H) % 64 == 0
    assert L.probe_lookup16(thr.ctypes.data, lut.ctypes.data, D.ctypes.data, cl.ctypes.data, out.ctypes.data, len(H) // 64) == 0
    return out


@pytest.mark.gpu
def test_gpu_lookups_equal_exact_count(gpu, host):
    """gfx950 qual_value == qual_value_lut (on the builder's table, and with every bucket flagged) == the exact count, every table and h"""
    for name, thr in all_class_tables():
        ex = exact(thr)
        lut = build_lut(host, thr)
        assert_same(qual_value(gpu, thr), ex, name + ": gfx950 qual_value")
        assert_same(qual_value_lut(gpu, thr, lut), ex, name + ": gfx950 qual_value_lut")
        assert_same(qual_value_lut(gpu, thr, lut | np.uint16(0x8000)), ex, name + ": gfx950 qual_value_lut, every bucket walked")


@pytest.mark.gpu
def test_gpu_lookup16_equals_exact_count(gpu, host):
    """qual_lookup16 on one wavefront per workgroup, tables in LDS, class words from cls_pack16 / cls_unpack4: every (h, class) of every
    table set, the ballot waves (no lane, one lane, every lane flagged), and the same with every bucket flagged"""
    rng = np.random.default_rng(4242)
    kinds_seen = set()
    for name, tabs in table_sets():
        ex = np.stack([exact(t) for t in tabs])
        luts = [build_lut(host, t) for t in tabs]
        for variant, lv in (("", luts), (", every bucket flagged", [lut | np.uint16(0x8000) for lut in luts])):
            H, Cl, kinds = lookup16_lanes(tabs, lv, rng)
            got = lookup16(gpu, tabs, lv, H, Cl)
            exp = ex[Cl, H]
            bad = np.nonzero(np.any(got != exp, axis=1))[0]
            if len(bad):
                ln = int(bad[0]); i = int(np.argmax(got[ln] != exp[ln]))
                raise AssertionError("%s%s: %d of %d lanes differ; first: wave %d (%s), lane %d, position %d, class %d, h = %d: %d against %d"
                                     % (name, variant, len(bad), len(H), ln // 64, kinds[ln // 64], ln % 64, i, int(Cl[ln, i]), int(H[ln, i]),
                                        int(got[ln, i]), int(exp[ln, i])))
            kinds_seen |= set(kinds)
    assert kinds_seen == {"all", "none", "one", "every"}
