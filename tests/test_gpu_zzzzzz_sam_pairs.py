"""GPU parity of the training side's SAM input ("SAM input: the line pairs"): ns_sam_pairs_build and ns_hp_histograms_sam
(k_sam_scan + k_sam_lines, csrc/ns_train.h) against what the REAL src/pairwise2maf.py wrote (tests/golden/reference_sam_pairs.json.gz) and
against the same walk compiled for the host.  (The file sorts behind every other -m gpu file: these are the newest kernels of the engine —
and for the same reason it runs in a CHILD pytest first, like tests/test_gpu_zzzz_hp_train.py: a device fault or a hang there fails this
file with the child's output, not the whole -m gpu run.)"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from nanosim_amd import characterize
from nanosim_amd import engine as E
from tests.test_hp_train import KS
from tests.test_sam_pairs import (BAD, HAND, SENTINEL, build_host_walk, check_bad_records, check_bleed, check_every_offset_and_length, check_fixture, check_sizing, lines_of, load_fixture,
                                  raw_build, rec, same)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORD, WAVE, BLOCK = 16, 1024, 4096          # what a thread, a wavefront and a workgroup of k_sam_lines write of each line


@pytest.fixture(scope="module")
def fx():
    return load_fixture()


@pytest.fixture(scope="module")
def host():
    return build_host_walk()


@pytest.fixture(scope="module")
def child_ok():
    if os.environ.get("NS_SAM_CHILD"):
        return
    try:
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider"], cwd=ROOT,
                           env=dict(os.environ, NS_SAM_CHILD="1"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    except subprocess.TimeoutExpired as ex:
        pytest.fail("the child run of this file did not finish in 300 s:\n" + str(ex.stdout or "")[-3000:])
    if r.returncode != 0:
        pytest.fail("the child run of this file failed (exit %d):\n%s" % (r.returncode, r.stdout[-4000:]))


@pytest.fixture(scope="module")
def eng(child_ok):
    e = E.Engine(0)
    yield e
    e.close()


def equal_to_host(eng, host, recs, **kw):
    """the raw call on the GPU and on the host: the same status, counters, offsets, figures and bytes (the sentinel included)"""
    g, h = raw_build(eng, recs, **kw), raw_build(host, recs, **kw)
    assert g[0] == h[0] == 0
    assert (g[1].n_bytes, g[1].n_bad, g[1].first_bad) == (h[1].n_bytes, h[1].n_bad, h[1].first_bad)
    for a, b in zip(g[2:], h[2:]):
        assert np.array_equal(a, b)
    return g


def test_gpu_fixture_lines_offsets_and_figures(fx, eng, host):
    """341 records: two workgroups of k_sam_scan, slots that begin at every offset mod 16"""
    assert len(fx["records"]) > 256
    off = check_fixture(eng, fx)
    assert set(int(o) % 16 for o in off[:-1]) == set(range(16))
    g = equal_to_host(eng, host, fx["records"])
    assert g[1].ms_kernel > 0
    packed = characterize.pairs_from_sam(eng, fx["records"])
    assert list(packed) == fx["tuples"] and packed.ref[-1] == 0 and packed.qry[-1] == 0
    assert characterize.format_maf(fx["records"], packed) == fx["maf"]


def sam_of_pair(ref, qry, head="", tail=""):
    """(CIGAR, MD, SEQ) of an aligned line pair"""
    ops, md, run, prev = [], [], 0, None
    for r, q in zip(ref, qry):
        op = "I" if r == "-" else "D" if q == "-" else "M"
        if ops and ops[-1][1] == op:
            ops[-1][0] += 1
        else:
            ops.append([1, op])
        if op == "M" and r == q:
            run += 1
        elif op == "M":
            md.append(str(run) + r)
            run = 0
        elif op == "D" and prev == "D":
            md[-1] += r
        elif op == "D":
            md.append(str(run) + "^" + r)
            run = 0
        prev = op
    cigar = ("%dS" % len(head) if head else "") + "".join("%d%s" % (n, op) for n, op in ops) + ("%dS" % len(tail) if tail else "")
    return cigar, "".join(md) + str(run), head + qry.replace("-", "") + tail


def random_pair(rng, n):
    """n columns: about 8 % each of inserted, deleted and substituted bases, never a dash over a dash"""
    base = np.frombuffer(b"ACGT", dtype=np.uint8)
    while True:
        u = rng.random(n)
        r, q = base[rng.integers(0, 4, n)].copy(), base[rng.integers(0, 4, n)].copy()
        q[u >= 0.24] = r[u >= 0.24]
        r[u < 0.08] = ord("-")
        q[(u >= 0.08) & (u < 0.16)] = ord("-")
        if (q != ord("-")).any():                 # (SAM cannot state a record without a base)
            return r.tobytes().decode(), q.tobytes().decode()


def check_pairs(eng, host, pairs, clips=None):
    """records derived from these pairs come back as these pairs, from the GPU as from the host"""
    recs = [rec(*sam_of_pair(r, q, *(clips[i] if clips else ("", "")))) for i, (r, q) in enumerate(pairs)]
    g = equal_to_host(eng, host, recs)
    assert g[1].n_bad == 0 and lines_of(g[2], g[3], g[4]) == list(pairs)
    assert (g[2][int(g[1].n_bytes):] == SENTINEL).all() and (g[3][int(g[1].n_bytes):] == SENTINEL).all()
    return g


def test_gpu_smallest_shapes_of_the_line_kernel(eng, host):
    rng = np.random.default_rng(7)
    # every length around a word and a wavefront's 64 words of columns, alone (the slot begins at 0) and in one call (it begins anywhere)
    sizes = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 5003)
    pairs = [random_pair(rng, n) for n in sizes]
    for p in pairs:
        check_pairs(eng, host, [p])
    clips = [("ACG" * (i % 3), "T" * (i % 5)) if p[0][0] != "-" and p[1][0] != "-" and p[0][-1] != "-" and p[1][-1] != "-" else ("", "")
             for i, p in enumerate(pairs)]
    check_pairs(eng, host, pairs, clips)
    check_pairs(eng, host, pairs[::-1])
    # a record whose only columns are one insertion run, lying across the border of a word, of a wavefront's KiB and of a workgroup's 4 KiB
    for border in (WORD, WAVE, BLOCK):
        front = ("A" * (border - 7), "A" * (border - 7))
        g = check_pairs(eng, host, [front, ("-" * 40, "ACGT" * 10), ("C" * 30, "C" * 30)])
        assert g[4].tolist() == [0, border - 7, border + 33, border + 63] and g[5].tolist()[1] == (0, 0, 0, 40)
    # a deletion run as the first op and one as the last op
    check_pairs(eng, host, [("ACGTTT", "---TTT"), ("TTTACG", "TTT---"), ("AC" + "G" * 40, "--" + "G" * 40), ("G" * 40 + "AC", "G" * 40 + "--")])
    # a mismatch in the last column of a word / a KiB / 4 KiB and one in the first column of the next
    r = np.full(BLOCK + 100, ord("A"), dtype=np.uint8)
    q = r.copy()
    for border in (WORD, WAVE, BLOCK):
        q[border - 1], q[border] = ord("c"), ord("G")
    check_pairs(eng, host, [(r.tobytes().decode(), q.tobytes().decode())])
    # 1-column records: sixteen and more of them in one word
    check_pairs(eng, host, [("A", "C") if i % 3 else ("-", "G") for i in range(70)])
    for row in HAND:
        g = equal_to_host(eng, host, [rec(*row[:3])])
        assert lines_of(g[2], g[3], g[4]) == [row[3:5]]


def test_gpu_40_records_in_index_order_and_a_call_of_3(fx, eng, host):
    for n in (40, 3):
        g = equal_to_host(eng, host, fx["records"][:n])
        assert lines_of(g[2], g[3], g[4]) == [tuple(x) for x in fx["lines"][:n]]
    check_sizing(eng, fx)


def test_gpu_bad_records_in_the_middle_of_a_call(eng, host):
    check_bad_records(eng, BAD)
    check_bleed(eng)                                             # (the packed device buffers: a neighbour's bytes really are adjacent)
    recs = [rec(c, m, s) for c, m, s in BAD if len(s) < 100]
    g = equal_to_host(eng, host, recs)
    assert g[1].n_bad == len(recs) and g[1].n_bytes == 0 and (g[2] == SENTINEL).all() and not g[5].view(np.uint32).any()


def test_gpu_md_strings_at_every_offset_and_length(eng):
    check_every_offset_and_length(eng)


@pytest.fixture(scope="module")
def host_counts(fx, host):
    """count_homopolymers of the host walk on the 341 pairs as tuples, per k, computed once"""
    return {k: characterize.count_homopolymers(host, fx["tuples"], k, records=True) for k in KS}


@pytest.mark.parametrize("k", KS)
def test_gpu_fused_call_equals_pairs_then_count_equals_the_host(fx, eng, host_counts, k):
    fused = characterize.count_homopolymers_sam(eng, fx["records"], k, records=True)
    assert fused["pairs"].ref is None and fused["ms_kernel"] > fused["ms_kernel_pairs"] > 0
    packed = characterize.pairs_from_sam(eng, fx["records"])
    two = characterize.count_homopolymers(eng, packed, k, records=True)
    assert same(fused, two) and same(two, host_counts[k])
    small = characterize.count_homopolymers_sam(eng, fx["records"], k, records=True, lines=True, cap_ref=2, cap_read=3, cap_records=5)
    assert same(small, host_counts[k]) and list(small["pairs"]) == fx["tuples"]


def test_gpu_fused_call_counts_nothing_when_a_record_is_bad(eng):
    t = characterize.NsHpHist()
    table = np.full((2, 8, 8), 7, dtype=np.uint64)
    t.cap_ref, t.cap_read, t.table = 8, 8, table.ctypes.data
    recs = [rec("6M", "6", "AAAAAA"), rec("4M", "5", "ACGT"), rec("6M", "6", "CCCCCC")]
    args, keep = characterize._pack_sam(recs)
    p, bufs = characterize._sam_out(recs, keep, True)
    assert eng.L.ns_hp_histograms_sam(eng.ctx, *args, 3, 5, C.byref(p), C.byref(t)) == 0
    assert (p.n_bad, p.first_bad, p.n_bytes, t.n_hp) == (1, 1, 12, 0) and not table.any() and t.columns[:] == [0, 0, 0, 0]
    assert bufs["off"].tolist() == [0, 6, 6, 12] and bufs["ref"][:12].tobytes() == b"AAAAAACCCCCC"
    assert eng.L.ns_hp_histograms_sam(eng.ctx, *args, 1, 5, None, C.byref(t)) == 0
    assert t.n_hp == 1 and table[0, 6, 6] == 1 and table.sum() == 1 and t.columns[:] == [0, 0, 0, 6]


def test_gpu_files_from_sam(fx, eng, host, tmp_path):
    for k in (5, 1):
        a, b = str(tmp_path / ("sam%d" % k)), str(tmp_path / ("maf%d" % k))
        characterize.homopolymer_lengths_from_sam(a, fx["records"], eng, min_hp_len=k, maf_file=True)
        characterize.homopolymer_lengths(b, fx["tuples"], eng, min_hp_len=k)
        for suffix in ("_hp_lengths.tsv", "_hp_lengths_model_parameters.tsv"):
            assert open(a + suffix).read() == open(b + suffix).read()
        assert open(a + "_processed.maf").read() == fx["maf"]


def test_gpu_two_calls_of_different_size_on_one_engine(fx, eng, host, host_counts):
    """scratch is per call: a small call, then a larger one, then the small one again"""
    e = E.Engine(0)
    try:
        for n in (3, 341, 3):
            g = equal_to_host(e, host, fx["records"][:n])
            assert lines_of(g[2], g[3], g[4]) == [tuple(x) for x in fx["lines"][:n]]
        assert same(characterize.count_homopolymers_sam(e, fx["records"][:3], 3, records=True),
                    characterize.count_homopolymers(host, fx["tuples"][:3], 3, records=True))
        assert same(characterize.count_homopolymers_sam(e, fx["records"], 3, records=True), host_counts[3])
    finally:
        e.close()


def test_gpu_no_records_and_argument_checks(eng):
    rc, p, ref, qry, off, aln = raw_build(eng, [])
    assert rc == 0 and (p.n_bytes, p.n_bad, p.first_bad) == (0, 0, 0) and off.tolist() == [0] and (ref == SENTINEL).all()
    t = characterize.count_homopolymers_sam(eng, [], 5, records=True)
    assert t["n_hp"] == 0 and not t["table"].any() and t["records"].shape == (0, 5)
    recs = [rec("4M", "4", "ACGT")]
    args, keep = characterize._pack_sam(recs)
    p, bufs = characterize._sam_out(recs, keep, True)
    down = np.array([3, 2], dtype=np.uint64)
    assert eng.L.ns_sam_pairs_build(eng.ctx, *args, 1, C.byref(p)) == 0 and bufs["ref"][:4].tobytes() == b"ACGT"
    for i in range(6):
        a = list(args)
        a[i] = None
        assert eng.L.ns_sam_pairs_build(eng.ctx, *a, 1, C.byref(p)) == E.NS_EINVAL, i
        assert b"ns_sam_pairs_build" in eng.L.ns_last_error(eng.ctx)
        if i % 2:
            a[i] = down.ctypes.data
            assert eng.L.ns_sam_pairs_build(eng.ctx, *a, 1, C.byref(p)) == E.NS_EINVAL, i
    assert eng.L.ns_sam_pairs_build(eng.ctx, *args, 1, None) == E.NS_EINVAL
    p.query_lines = None
    assert eng.L.ns_sam_pairs_build(eng.ctx, *args, 1, C.byref(p)) == E.NS_EINVAL
    p.ref_lines, p.aln_off = None, None
    assert eng.L.ns_sam_pairs_build(eng.ctx, *args, 1, C.byref(p)) == E.NS_EINVAL
    h = characterize.NsHpHist()
    table = np.zeros((2, 8, 8), dtype=np.uint64)
    h.cap_ref, h.cap_read, h.table = 8, 8, table.ctypes.data
    assert eng.L.ns_hp_histograms_sam(eng.ctx, *args, 1, 0, None, C.byref(h)) == E.NS_EINVAL
    assert b"ns_hp_histograms_sam" in eng.L.ns_last_error(eng.ctx)
    assert eng.L.ns_hp_histograms_sam(eng.ctx, *args, 1, 5, None, None) == E.NS_EINVAL
    h.table = None
    assert eng.L.ns_hp_histograms_sam(eng.ctx, *args, 1, 5, None, C.byref(h)) == E.NS_EINVAL
