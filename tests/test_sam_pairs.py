"""Training side, SAM input ("SAM input: the line pairs") on CPU: the engine's walk over CIGAR, MD and SEQ
(nanosim_amd/csrc/ns_sam_pairs.h, compiled for the host; on the GPU k_sam_scan and k_sam_lines of ns_train.h run it) and the host module
around the calls — pinned against what the REAL src/pairwise2maf.py wrote for the same records (tests/golden/reference_sam_pairs.json.gz,
tests/golden/make_sam_pairs_golden.py), against the homopolymer fixture the records were derived from, and against hand-made records."""
import ctypes as C
import gzip
import json
import os
import re
import subprocess
import types

import numpy as np
import pytest

from nanosim_amd import characterize, engine
from tests.test_hp_train import KS, expected_table
from tests.test_hp_train import load_fixture as load_hp_fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0xA5


def load_fixture():
    with gzip.open(os.path.join(ROOT, "tests", "golden", "reference_sam_pairs.json.gz"), "rt") as f:
        fx = json.load(f)
    fx["records"] = [tuple(r) for r in fx["records"]]
    fx["tuples"] = [(r[2], r[3] - 1, a, b) for r, (a, b) in zip(fx["records"], fx["lines"])]
    return fx


@pytest.fixture(scope="module")
def fx():
    return load_fixture()


def build_host_walk():
    """an object that stands in for an Engine: its SAM calls and its ns_hp_histograms are the engine's walks compiled for the host
    (tests/sam_pairs_host.cpp)"""
    out = os.path.join(ROOT, "tests", "_tmp")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libsam_pairs_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tests", "sam_pairs_host.cpp")])
    L = C.CDLL(so)
    L.sam_host_pairs_build.restype = C.c_int
    L.sam_host_pairs_build.argtypes = [C.c_void_p] + [C.c_void_p] * 6 + [C.c_uint32, C.c_void_p]
    L.sam_host_hp_histograms_sam.restype = C.c_int
    L.sam_host_hp_histograms_sam.argtypes = [C.c_void_p] + [C.c_void_p] * 6 + [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    L.hp_host_histograms.restype = C.c_int
    L.hp_host_histograms.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]

    def check(rc):
        if rc:
            raise engine.EngineError("host walk: error %d" % rc)
    return types.SimpleNamespace(ctx=None, _check=check, L=types.SimpleNamespace(
        ns_sam_pairs_build=L.sam_host_pairs_build, ns_hp_histograms_sam=L.sam_host_hp_histograms_sam, ns_hp_histograms=L.hp_host_histograms))


@pytest.fixture(scope="module")
def host():
    return build_host_walk()


def rec(cigar, md, seq, flag=0, name="r", rname="chr1", pos=1):
    return (name, flag, rname, pos, cigar, md, seq)


def raw_build(eng, recs, cap=None, lines=True, extra=64):
    """ns_sam_pairs_build on buffers filled with the sentinel byte: (rc, the struct, reference bytes, query bytes, offsets, figures);
    cap: cap_bytes (None: what no record can exceed); the line buffers hold `extra` bytes more than cap_bytes"""
    args, keep = characterize._pack_sam(recs)
    n = len(recs)
    if cap is None:
        cap = int(keep[3][-1]) + int(keep[5][-1])
    p = characterize.NsSamPairs()
    ref = np.full(cap + extra, SENTINEL, dtype=np.uint8)
    qry = np.full(cap + extra, SENTINEL, dtype=np.uint8)
    off = np.full(n + 1, 0xA5A5A5A5, dtype=np.uint64)
    aln = np.full(4 * n, 0xA5A5A5A5, dtype=np.uint32).view(characterize.SAM_ALN_DTYPE)
    p.aln_off, p.aln, p.cap_bytes = off.ctypes.data, aln.ctypes.data if n else None, cap
    if lines:
        p.ref_lines, p.query_lines = ref.ctypes.data, qry.ctypes.data
    rc = eng.L.ns_sam_pairs_build(eng.ctx, *args, n, C.byref(p))
    return rc, p, ref, qry, off, aln


def lines_of(ref, qry, off):
    return [(ref[int(a):int(b)].tobytes().decode(), qry[int(a):int(b)].tobytes().decode()) for a, b in zip(off[:-1], off[1:])]


def check_fixture(eng, fx):
    """lines, offsets and figures of the 341 records against the fixture; the sentinel behind n_bytes"""
    rc, p, ref, qry, off, aln = raw_build(eng, fx["records"])
    assert rc == 0 and p.n_bad == 0 and p.first_bad == len(fx["records"])
    exp_off = np.cumsum([0] + [len(a) for a, _ in fx["lines"]])
    assert np.array_equal(off, exp_off) and p.n_bytes == exp_off[-1]
    assert lines_of(ref, qry, off) == [tuple(x) for x in fx["lines"]]
    assert [list(map(int, a)) for a in aln.tolist()] == fx["figures"]
    assert (ref[int(p.n_bytes):] == SENTINEL).all() and (qry[int(p.n_bytes):] == SENTINEL).all()
    return off


def test_host_lines_offsets_and_figures_equal_the_fixture(fx, host):
    assert len(fx["records"]) == 341 > 256
    off = check_fixture(host, fx)
    assert set(int(o) % 16 for o in off[:-1]) == set(range(16))
    packed = characterize.pairs_from_sam(host, fx["records"])
    assert len(packed) == 341 and list(packed) == fx["tuples"] and packed[7] == fx["tuples"][7] and packed[-1] == fx["tuples"][-1]
    assert packed.ref[-1] == 0 and packed.qry[-1] == 0 and len(packed.ref) == int(packed.off[-1]) + 1
    assert characterize._pack_pairs(packed)[0] is packed.ref


def test_format_maf_equals_the_reference(fx, host, tmp_path):
    packed = characterize.pairs_from_sam(host, fx["records"])
    assert characterize.format_maf(fx["records"], packed) == fx["maf"]
    characterize.write_maf(str(tmp_path / "x.maf"), fx["records"], packed)
    assert open(str(tmp_path / "x.maf")).read() == fx["maf"]
    assert characterize.maf_records(str(tmp_path / "x.maf")) == fx["tuples"]


@pytest.fixture(scope="module")
def tuple_counts(fx, host):
    """count_homopolymers on the 341 pairs as tuples, per k, computed once (the GPU tests share it)"""
    return {k: characterize.count_homopolymers(host, fx["tuples"], k, records=True) for k in KS}


def same(a, b):
    return (a["table"].shape == b["table"].shape and np.array_equal(a["table"], b["table"]) and np.array_equal(a["columns"], b["columns"])
            and a["n_hp"] == b["n_hp"] and np.array_equal(a["records"], b["records"]))


@pytest.mark.parametrize("k", KS)
def test_counts_on_packed_pairs_equal_counts_on_tuples_and_the_reference(fx, host, tuple_counts, k):
    packed = characterize.pairs_from_sam(host, fx["records"])
    t = characterize.count_homopolymers(host, packed, k, records=True)
    assert same(t, tuple_counts[k])
    # ... and the reference's table for all 414 pairs.  The 66 pairs without columns hold no homopolymer; the 7 whose query line is only
    # dashes do when k is small (a reference letter over a dash is a homopolymer of read length 0 at k = 1): their counts, from the
    # tuple path, are added before the comparison, and at k = 5 they are none
    hp = load_hp_fixture()
    left_out = [r for i, r in enumerate(hp["records"]) if i not in set(fx["source_index"])]
    assert len(left_out) == 73 and sum(1 for r in left_out if not r[2]) == 66
    rest = characterize.count_homopolymers(host, left_out, k)
    exp = expected_table(hp, k)
    total = np.zeros_like(exp)
    total[:, :t["table"].shape[1], :t["table"].shape[2]] += t["table"]
    total[:, :rest["table"].shape[1], :rest["table"].shape[2]] += rest["table"]
    assert np.array_equal(total, exp) and (k < 5 or rest["n_hp"] == 0)
    fused = characterize.count_homopolymers_sam(host, fx["records"], k, records=True, cap_ref=2, cap_read=3, cap_records=5)
    assert same(fused, t) and fused["pairs"].ref is None


def host_maf(host):
    """a stand-in whose ns_maf_histograms only records what reaches it"""
    def fake(ctx, ref, qry, nbytes, off, n, h):
        fake.seen = (ref, qry, nbytes, n)
        return 0
    return types.SimpleNamespace(ctx=None, _check=host._check, L=types.SimpleNamespace(ns_maf_histograms=fake))


def test_count_maf_takes_packed_pairs_as_they_are(fx, host):
    packed = characterize.pairs_from_sam(host, fx["records"])
    e = host_maf(host)
    characterize.count_maf(e, packed)
    assert e.L.ns_maf_histograms.seen == (packed.ref.ctypes.data, packed.qry.ctypes.data, int(packed.off[-1]), 341)


HAND = [   # CIGAR, MD, SEQ, reference line, query line, (head, tail, ref_len, query_len)
    ("3=1X2=", "3A2", "ACGTAC", "ACGAAC", "ACGTAC", (0, 0, 6, 6)),                      # = / X ops
    ("2H3S4M1S5H", "4", "TTTACGTA", "ACGT", "ACGT", (3, 1, 4, 4)),                      # H outside S
    ("2M2D2M", "2^AC0T1", "GGCA", "GGACTA", "GG--CA", (0, 0, 6, 4)),                    # 0 between a ^ run and a mismatch
    ("2M1D2I2D2M", "2^ACG2", "GGTTCA", "GGA--CGCA", "GG-TT--CA", (0, 0, 7, 6)),         # one ^ run over D, I, D
    ("1M4D1M", "1^AC0^GT1", "TT", "TACGTT", "T----T", (0, 0, 6, 2)),                    # two ^ runs, a 0 between them, one D
    ("6I", "0", "ACGTAA", "------", "ACGTAA", (0, 0, 0, 6)),                            # 6I with MD 0
    ("4M", "1a1n0", "ACGT", "AaGn", "ACGT", (0, 0, 4, 4)),                              # lower-case MD letters
    ("5S1M7S", "1", "AAAAACTTTTTTT", "C", "C", (5, 7, 1, 1)),                           # all clip plus one M
    ("2M3I1M", "0C0G1", "TTAAAG", "CG---G", "TTAAAG", (0, 0, 3, 6)),                    # mismatches in front of an insertion
    ("1D3M", "0^T3", "ACG", "TACG", "-ACG", (0, 0, 4, 3)),                              # a deletion as the first op
    ("3M2D", "3^gt0", "ACG", "ACGgt", "ACG--", (0, 0, 5, 3)),                           # ... and as the last op
    ("4M", "1z1Z0", "ACGT", "AzGZ", "ACGT", (0, 0, 4, 4)),                              # the last letters of both alphabets, as mismatches
    ("1M4D1M", "1^zZAa1", "CG", "CzZAaG", "C----G", (0, 0, 6, 2)),                      # ... and the first, in a ^ run
]


def test_hand_cases(host):
    recs = [rec(c, m, s) for c, m, s, _, _, _ in HAND]
    rc, p, ref, qry, off, aln = raw_build(host, recs)
    assert rc == 0 and p.n_bad == 0
    assert lines_of(ref, qry, off) == [(r, q) for _, _, _, r, q, _ in HAND]
    assert [tuple(map(int, a)) for a in aln.tolist()] == [f for *_, f in HAND]
    assert (ref[int(p.n_bytes):] == SENTINEL).all() and (qry[int(p.n_bytes):] == SENTINEL).all()
    for i in range(len(recs)):                                   # each one alone: another place in the buffers
        rc, p, ref, qry, off, aln = raw_build(host, recs[i:i + 1])
        assert rc == 0 and p.n_bad == 0 and lines_of(ref, qry, off) == [HAND[i][3:5]]


BIG = 1 << 24
BAD = [   # CIGAR, MD, SEQ: every kind of bad record
    ("2M1N2M", "4", "ACGT"), ("4P", "4", "ACGT"), ("4Q", "4", "ACGT"), ("4", "4", "ACGT"), ("M", "1", "A"),      # an op outside MIDSH=X, no op, no number
    ("2M1S2M", "4", "ACGTA"), ("1S1H3M", "3", "ACGT"), ("3M1H1S", "3", "ACGT"), ("1S1S3M", "3", "ACGTA"),       # S not outermost
    ("1H1H3M", "3", "ACG"),
    ("", "4", "ACGT"), ("*", "4", "ACGT"), ("4M", "4", ""), ("4M", "4", "*"),                                       # CIGAR / SEQ empty or *
    ("4M", "4", "ACG"), ("4M", "4", "ACGTA"), ("1S4M", "4", "ACGT"), ("2M2I", "2", "ACG"),                          # SEQ's length
    ("4M", "2^A2", "ACGT"), ("2M1D1M", "2^AC1", "ACG"),                                                             # an M column meets a ^ letter
    ("2M1D2M", "5", "ACGT"), ("2M1D2M", "2A2", "ACGT"), ("2M2D2M", "2^A2", "ACGT"), ("2M1D2M", "2^2", "ACGT"),      # a D column meets anything else
    ("4M", "3", "ACGT"), ("4M", "2A", "ACGT"), ("4M", "", "ACGT"), ("2M1D2M", "2", "ACGT"),                         # MD ends early
    ("4M", "5", "ACGT"), ("4M", "4A0", "ACGT"), ("4M", "4^A0", "ACGT"), ("4M", "A3", "ACGT"), ("4M", "4 ", "ACGT"),  # MD has items left over / is no MD
    ("%dM" % BIG, "%d" % BIG, "A" * BIG),                                                                           # 2^24 columns
    # a second trailing S — with a SEQ that fits the last S alone, with one that fits both —, an S behind the trailing H, a second leading S
    ("4M2S3S", "4", "ACGTCCC"), ("4M2S3S", "4", "ACGTTTCCC"), ("4M2H3S", "4", "ACGTCCC"), ("4M2S1H3S", "4", "ACGTTTCCC"), ("2S3S4M", "4", "CCCACGT"),
    # an MD that ends where its next number has to stand, in front of a record whose MD begins with a digit (check_bad_records: `2^GG3`)
    ("2I", "", "AC"), ("3M", "2A", "ACG"), ("2M1D", "2^A", "AC"), ("1M2I1M", "0T", "ACGT"),
]


def check_bad_records(eng, records):
    """every bad record between two good ones: zero columns, all-zero figures, the right first_bad, the neighbours' bytes as they are
    without it, the sentinel behind n_bytes"""
    good = [rec("3S5M", "2a2", "TTTACGTA"), rec("2M2D2M1I1M", "2^GG3", "ACGTTA"), rec("1M", "1", "N")]
    rc, p, ref, qry, off, aln = raw_build(eng, good)
    assert rc == 0 and p.n_bad == 0
    exp = lines_of(ref, qry, off)
    assert exp == [("ACaTA", "ACGTA"), ("ACGGGT-A", "AC--GTTA"), ("N", "N")]
    exp_aln = aln.tolist()
    for c, m, s in records:
        recs = [good[0], rec(c, m, s), good[1], good[2]]
        rc, p, ref, qry, off, aln = raw_build(eng, recs)
        assert rc == 0 and (p.n_bad, p.first_bad) == (1, 1), (c, m, s[:10])
        assert off.tolist() == [0, 5, 5, 13, 14] and p.n_bytes == 14
        got = lines_of(ref, qry, off)
        assert got == [exp[0], ("", ""), exp[1], exp[2]], (c, m, s[:10])
        assert aln.tolist() == [exp_aln[0], (0, 0, 0, 0), exp_aln[1], exp_aln[2]]
        assert (ref[14:] == SENTINEL).all() and (qry[14:] == SENTINEL).all()
    # several in one call, the first one counts
    recs = [good[0]] + [rec(*records[0]), good[1], rec(*records[1]), rec(*records[2]), good[2]]
    rc, p, ref, qry, off, aln = raw_build(eng, recs)
    assert rc == 0 and (p.n_bad, p.first_bad) == (3, 1) and lines_of(ref, qry, off) == [exp[0], ("", ""), exp[1], ("", ""), ("", ""), exp[2]]
    with pytest.raises(ValueError, match="first is record 1 "):
        characterize.pairs_from_sam(eng, recs)


# The strings of a call lie one behind the other: a walk that looks one byte too far sees the FIRST byte of the next record's string.
# Every case: records whose CIGAR or MD ends early, each directly in front of a neighbour whose string begins with what the walk would
# have wanted next; (records, which of them are good).  The bad one stays bad and the neighbour is judged on its own.
BLEED = [
    # MD ends one item early; the neighbour's MD begins with a letter (itself no MD), with `^X` (itself no MD), with a digit (a good one)
    ([("4M", "2", "ACGT"), ("4M", "A3", "ACGT")], [False, False]),
    ([("4M", "2", "ACGT"), ("4M", "4", "ACGT")], [False, True]),
    ([("2M1D2M", "2", "ACGT"), ("2M1D2M", "^A4", "ACGT")], [False, False]),
    ([("2M1D2M", "2^", "ACGT"), ("4M", "A3", "ACGT")], [False, False]),
    ([("2M2D1M", "2^A", "ACG"), ("4M", "C3", "ACGT")], [False, False]),
    ([("2M1D", "2^A", "AC"), ("4M", "C3", "ACGT")], [False, False]),
    ([("2M1D", "2^A", "AC"), ("4M", "4", "ACGT")], [False, True]),
    ([("3M", "2A", "ACG"), ("4M", "4", "ACGT")], [False, True]),
    ([("3M", "2A", "ACG"), ("2M1D2M", "2^G2", "ACGT")], [False, True]),
    ([("2I", "", "AC"), ("4M", "4", "ACGT")], [False, True]),
    ([("2I", "", "AC"), ("2I", "0", "AC")], [False, True]),
    ([("4M", "1", "ACGT"), ("3M", "3", "ACG")], [False, True]),                          # (1 + 3 would be the four columns)
    # CIGAR: a count without an op; the neighbour's CIGAR begins with an op letter (itself no CIGAR), or with a digit
    ([("4", "4", "ACGT"), ("M", "1", "A")], [False, False]),
    ([("4", "4", "ACGT"), ("M4M", "4", "ACGT")], [False, False]),
    ([("2M2", "4", "ACGT"), ("I1M", "1", "A")], [False, False]),
    ([("2M2", "4", "ACGT"), ("2M", "2", "AC")], [False, True]),
    ([("4", "4", "ACGT"), ("4M", "4", "ACGT")], [False, True]),
]
BLEED_LINES = {("4M", "4", "ACGT"): ("ACGT", "ACGT"), ("2M1D2M", "2^G2", "ACGT"): ("ACGGT", "AC-GT"), ("2I", "0", "AC"): ("--", "AC"),
               ("3M", "3", "ACG"): ("ACG", "ACG"), ("2M", "2", "AC"): ("AC", "AC")}


def check_bleed(eng):
    """every BLEED case alone between `H S .. S H` and a plain record, then all of them in one call: the verdicts, the lines and the figures"""
    first, last = rec("2H3S4M1S5H", "4", "TTTACGTA"), rec("1M", "1", "N")
    def expect(records, good):
        return [("ACGT", "ACGT")] + [BLEED_LINES[r] if g else ("", "") for r, g in zip(records, good)] + [("N", "N")]
    everything, verdicts = [], []
    for records, good in BLEED:
        assert all(r in BLEED_LINES for r, g in zip(records, good) if g)
        rc, p, ref, qry, off, aln = raw_build(eng, [first] + [rec(*r) for r in records] + [last])
        assert rc == 0 and lines_of(ref, qry, off) == expect(records, good), records
        bad = [i + 1 for i, g in enumerate(good) if not g]
        assert (p.n_bad, p.first_bad) == (len(bad), bad[0]), records
        assert [tuple(map(int, a)) for a in aln.tolist()][0] == (3, 1, 4, 4) and all(tuple(map(int, aln[i])) == (0, 0, 0, 0) for i in bad)
        assert (ref[int(p.n_bytes):] == SENTINEL).all() and (qry[int(p.n_bytes):] == SENTINEL).all()
        everything += records
        verdicts += good
    rc, p, ref, qry, off, aln = raw_build(eng, [first] + [rec(*r) for r in everything] + [last])
    assert rc == 0 and lines_of(ref, qry, off) == expect(everything, verdicts) and p.n_bad == verdicts.count(False) and p.first_bad == 1


def md_record(n, letters="ACGazZ"):
    """an M-only record whose MD has n bytes: `1` or `10`, then n // 2 (less one) pairs of a letter and `1`; n == 0: an empty MD, a bad record"""
    md = ("1" if n % 2 else "10" if n else "") + "".join(letters[k % len(letters)] + "1" for k in range((n - 1) // 2))
    cols = sum(int(t) if t.isdigit() else 1 for t in re.findall(r"\d+|[A-Za-z]", md)) or 3
    assert len(md) == n
    return ("%dM" % cols, md, "T" * cols)


def plain_lines(md, seq):
    """the two lines of an M-only record, from its MD alone: digits copy SEQ, a letter stands in the reference line"""
    ref, i = [], 0
    for t in re.findall(r"\d+|[A-Za-z]", md):
        ref.append(seq[i:i + int(t)] if t.isdigit() else t)
        i += int(t) if t.isdigit() else 1
    return "".join(ref), seq


def check_every_offset_and_length(eng):
    """one call in which an MD of every length 0 .. 17 begins at every offset 0 .. 7 mod 8 of the packed MD bytes (the device reads
    CIGAR, MD and SEQ through aligned 8-byte windows); the CIGARs, two or three bytes each, come by every offset on the way"""
    recs, at, where = [], 0, []
    for n in range(18):
        for o in range(8):
            if at % 8 != o:
                recs.append(md_record((o - at) % 8, "C"))
                at += len(recs[-1][1])
            where.append(len(recs))
            recs.append(md_record(n))
            at += n
    md_off = np.cumsum([0] + [len(r[1]) for r in recs])
    cg_off = np.cumsum([0] + [len(r[0]) for r in recs])
    assert {(int(md_off[i]) % 8, len(recs[i][1])) for i in where} == {(o, n) for o in range(8) for n in range(18)}
    assert {int(o) % 8 for o in cg_off[:-1]} == set(range(8))
    want = [plain_lines(m, q) if m else ("", "") for _, m, q in recs]
    for order in (recs, recs[::-1]):
        rc, p, ref, qry, off, aln = raw_build(eng, [rec(*r) for r in order])
        assert rc == 0 and p.n_bad == 8 and lines_of(ref, qry, off) == (want if order is recs else want[::-1])
        assert [tuple(map(int, a)) for a in aln.tolist()] == [(0, 0, len(q), len(q)) if m else (0, 0, 0, 0) for _, m, q in order]
        assert (ref[int(p.n_bytes):] == SENTINEL).all() and (qry[int(p.n_bytes):] == SENTINEL).all()


def test_md_strings_at_every_offset_and_length(host):
    check_every_offset_and_length(host)


def test_a_string_that_ends_early_does_not_borrow_from_its_neighbour(host):
    check_bleed(host)


def test_bad_records(host):
    check_bad_records(host, BAD)
    # one column below the limit is a record like any other
    rc, p, ref, qry, off, aln = raw_build(host, [rec("%dM" % (BIG - 1), "%d" % (BIG - 1), "C" * (BIG - 1))], extra=1)
    assert rc == 0 and p.n_bad == 0 and p.n_bytes == BIG - 1 and (ref[:BIG - 1] == ord("C")).all() and ref[BIG - 1] == SENTINEL
    # a call whose records are bad counts nothing
    t = characterize.NsHpHist()
    table = np.full((2, 8, 8), 7, dtype=np.uint64)
    t.cap_ref, t.cap_read, t.table = 8, 8, table.ctypes.data
    recs = [rec("6M", "6", "AAAAAA"), rec("4M", "5", "ACGT")]
    args, keep = characterize._pack_sam(recs)
    p, bufs = characterize._sam_out(recs, keep, False)
    assert host.L.ns_hp_histograms_sam(None, *args, 2, 5, C.byref(p), C.byref(t)) == 0
    assert (p.n_bad, p.first_bad, t.n_hp) == (1, 1, 0) and not table.any()
    with pytest.raises(ValueError, match="first is record 1 "):
        characterize.count_homopolymers_sam(host, recs, 5)


def check_sizing(eng, fx):
    """the call with NULL lines sizes the buffers; one byte short writes no line; exactly enough writes them"""
    some = fx["records"][:40]
    n = sum(len(a) for a, _ in fx["lines"][:40])
    rc, p, ref, qry, off, aln = raw_build(eng, some, cap=0, lines=False)
    assert rc == 0 and p.n_bytes == n == off[-1] and [list(map(int, a)) for a in aln.tolist()] == fx["figures"][:40]
    assert (ref == SENTINEL).all() and (qry == SENTINEL).all()
    rc, p, ref, qry, off2, aln = raw_build(eng, some, cap=n - 1)
    assert rc == 0 and p.n_bytes == n and np.array_equal(off2, off) and (ref == SENTINEL).all() and (qry == SENTINEL).all()
    rc, p, ref, qry, off2, aln = raw_build(eng, some, cap=n, extra=3)
    assert rc == 0 and lines_of(ref, qry, off2) == [tuple(x) for x in fx["lines"][:40]] and (ref[n:] == SENTINEL).all() and (qry[n:] == SENTINEL).all()


def test_sizing_call_and_a_cap_one_byte_short(fx, host):
    check_sizing(host, fx)


def test_no_records(host):
    rc, p, ref, qry, off, aln = raw_build(host, [])
    assert rc == 0 and (p.n_bytes, p.n_bad, p.first_bad) == (0, 0, 0) and off.tolist() == [0] and (ref == SENTINEL).all()
    packed = characterize.pairs_from_sam(host, [])
    assert len(packed) == 0 and list(packed) == [] and packed.ref.tolist() == [0]
    assert characterize.format_maf([], packed) == ""
    t = characterize.count_homopolymers(host, packed, 5, records=True)
    assert t["n_hp"] == 0 and not t["table"].any()


def test_struct_layout_and_exports():
    src = r'''#include <stdio.h>
#include <stddef.h>
#include "nanosim_amd.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(ns_sam_pairs), offsetof(ns_sam_pairs, ref_lines), offsetof(ns_sam_pairs, query_lines),
         offsetof(ns_sam_pairs, cap_bytes), offsetof(ns_sam_pairs, aln_off), offsetof(ns_sam_pairs, aln), offsetof(ns_sam_pairs, n_bytes),
         offsetof(ns_sam_pairs, n_bad), offsetof(ns_sam_pairs, first_bad), offsetof(ns_sam_pairs, ms_kernel));
  printf("%zu %zu %zu %zu %zu\n", sizeof(ns_sam_aln), offsetof(ns_sam_aln, head), offsetof(ns_sam_aln, tail), offsetof(ns_sam_aln, ref_len),
         offsetof(ns_sam_aln, query_len));
  return 0; }'''
    out = os.path.join(ROOT, "tests", "_tmp")
    os.makedirs(out, exist_ok=True)
    c = os.path.join(out, "sam_layout.c")
    with open(c, "w") as f:
        f.write(src)
    exe = os.path.join(out, "sam_layout")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, c])
    a, b = subprocess.check_output([exe], text=True).strip().split("\n")
    P = characterize.NsSamPairs
    assert [int(v) for v in a.split()] == [C.sizeof(P), P.ref_lines.offset, P.query_lines.offset, P.cap_bytes.offset, P.aln_off.offset, P.aln.offset,
                                           P.n_bytes.offset, P.n_bad.offset, P.first_bad.offset, P.ms_kernel.offset]
    D = characterize.SAM_ALN_DTYPE
    assert [int(v) for v in b.split()] == [D.itemsize] + [D.fields[n][1] for n in ("head", "tail", "ref_len", "query_len")] == [16, 0, 4, 8, 12]
    assert "ns_sam_pairs_build" in engine.EXPORTS and "ns_hp_histograms_sam" in engine.EXPORTS


SAM_TEXT = "\n".join([
    "@HD\tVN:1.6\tSO:unsorted", "@SQ\tSN:chr1\tLN:5000",
    "r1\t0\tchr1\t101\t60\t2S4M\t*\t0\t0\tTTACGT\tIIIIII\tNM:i:0\tMD:Z:4\tcs:Z::4",
    "r2\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\tIIII",
    "r3\t16\tchr1\t7\t60\t2M1D2M\t*\t0\t0\tACGT\t*\tMD:Z:2^G2",
    "r4\t256\tchr1\t9\t0\t4M\t*\t0\t0\tACGT\tIIII\tMD:Z:4",
    "r5\t2048\tchr1\t9\t0\t4M\t*\t0\t0\tACGT\tIIII\tMD:Z:4",
    "r6\t2064\tchr1\t9\t0\t4M\t*\t0\t0\tACGT\tIIII\tMD:Z:4",
    "r7\t0\tchr2\t1\t60\t1M2I1M\t*\t0\t0\tACGT\tIIII\tMD:Z:0T1"]) + "\n"


def test_sam_records(tmp_path, host):
    p = tmp_path / "x.sam"
    p.write_text(SAM_TEXT)
    recs = characterize.sam_records(str(p))
    assert recs == [("r1", 0, "chr1", 101, "2S4M", "4", "TTACGT"), ("r3", 16, "chr1", 7, "2M1D2M", "2^G2", "ACGT"),
                    ("r7", 0, "chr2", 1, "1M2I1M", "0T1", "ACGT")]
    packed = characterize.pairs_from_sam(host, recs)
    assert list(packed) == [("chr1", 100, "ACGT", "ACGT"), ("chr1", 6, "ACGGT", "AC-GT"), ("chr2", 0, "T--T", "ACGT")]
    assert characterize.format_maf(recs, packed) == ("s chr1 100 4 + * ACGT\ns r1 2 4 + 6 ACGT\ns chr1 6 5 + * ACGGT\ns r3 0 4 - 4 AC-GT\n"
                                                     "s chr2 0 2 + * T--T\ns r7 0 4 + 4 ACGT\n")
    p.write_text(SAM_TEXT + "r8\t16\tchr1\t9\t0\t4M\t*\t0\t0\tACGT\tIIII\tNM:i:0\n")
    with pytest.raises(ValueError, match="r8 has no MD"):
        characterize.sam_records(str(p))
    p.write_text(SAM_TEXT + "r9\t0\tchr1\t9\t0\t2H4M\t*\t0\t0\tACGT\tIIII\tMD:Z:4\n")
    with pytest.raises(ValueError, match="r9 has a hard clip"):
        characterize.sam_records(str(p))


def test_files_from_sam_equal_files_from_the_pairs(fx, host, tmp_path):
    for k in (5, 1):
        a, b = str(tmp_path / ("sam%d" % k)), str(tmp_path / ("maf%d" % k))
        characterize.homopolymer_lengths_from_sam(a, fx["records"], host, min_hp_len=k, maf_file=True)
        characterize.homopolymer_lengths(b, fx["tuples"], host, min_hp_len=k)
        for suffix in ("_hp_lengths.tsv", "_hp_lengths_model_parameters.tsv"):
            assert open(a + suffix).read() == open(b + suffix).read()
        assert open(a + "_processed.maf").read() == fx["maf"]
    assert open(str(tmp_path / "sam5_hp_lengths.tsv")).read() == load_hp_fixture()["k"]["5"]["lengths_file"]
