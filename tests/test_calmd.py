"""cs and MD tags from the reference genome without a GPU ("cs and MD from the reference"): the engine's walks compiled for the
host with one lane (tests/calmd_host.cpp over nanosim_amd/csrc/ns_calmd.h, behind the signature of ns_calmd) against the independent
column-by-column writer and the generator of tests/calmd_lib.py, and against texts written out here; the Python side
(nanosim_amd/characterize/calmd.py) on that stand-in engine.  The check_* functions take an engine: tests/test_gpu_zzzzzzzzzz_calmd.py
runs them on the GPU."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest

from nanosim_amd import characterize, engine, model
from tests import bam_lib, calmd_lib
from tests.calmd_lib import write_tags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = calmd_lib.reference()
CHROMS = calmd_lib.chromosomes(REF)
LANES = 64


def build_host(lanes: int = 1):
    """an object that stands in for an Engine: its ns_calmd is the engine's per-wavefront code compiled for the host with one lane (or,
    lanes = 64, on the lock-step wavefront of tests/wave64_host.h), its set_reference keeps a copy normalised as the engine's"""
    out = os.path.join(ROOT, "tests", "_tmp")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libcalmd_host.so" if lanes == 1 else "libcalmd_host%d.so" % lanes)
    mine = "%s.%d" % (so, os.getpid())                               # (built under a name of its own and moved: test processes may run side by side)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-DCALMD_HOST_LANES=%d" % lanes, "-o", mine,
                           os.path.join(ROOT, "tests", "calmd_host.cpp")])
    os.replace(mine, so)
    L = C.CDLL(so)
    L.calmd_host.restype = C.c_int
    L.calmd_host.argtypes = [C.c_void_p] + [C.c_void_p] * 6 + [C.c_uint32, C.c_void_p]
    L.calmd_host_set_reference.restype = C.c_int
    L.calmd_host_set_reference.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32]
    L.calmd_host_guard.restype = C.c_int
    L.calmd_host_guard.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint32]
    L.calmd_host_constant.restype = C.c_uint32
    L.calmd_host_constant.argtypes = [C.c_int]

    def check(rc):
        if rc:
            err = engine.EngineError("calmd_host returned %d" % rc)
            err.code = rc
            raise err

    def set_reference(ref):
        check(L.calmd_host_set_reference(ref.bases.ctypes.data, len(ref.bases), ref.chrom_off.ctypes.data, len(ref.names)))
    return types.SimpleNamespace(ctx=None, _check=check, L=types.SimpleNamespace(ns_calmd=L.calmd_host), constant=L.calmd_host_constant,
                                 set_reference=set_reference, guard=L.calmd_host_guard)


@pytest.fixture(scope="module")
def host():
    h = build_host()
    h.set_reference(REF)
    return h


def tags(eng, records):
    """[(md, cs)] of (cigar, seq, chrom, pos) records, one call"""
    r = characterize.cs_md_call(eng, [x[0] for x in records], [x[1] for x in records], [x[2] for x in records], [x[3] for x in records])
    assert r["md_off"][0] == 0 and r["cs_off"][0] == 0 and len(r["md_off"]) == len(records) + 1
    return list(zip(characterize.texts_of(r, "md"), characterize.texts_of(r, "cs")))


# ---- cases written out by hand -------------------------------------------------------------------------------------------------------
def mut(b):
    return {"A": "C", "C": "G", "G": "T", "T": "A"}.get(b, "A")


def clean_window(chrom: str, size: int, last: bool = False) -> int:
    """where a stretch of `size` letters of ACGT only begins (the first one, or the last)"""
    it = range(len(chrom) - size, -1, -1) if last else range(0, len(chrom) - size)
    for o in it:
        if set(chrom[o:o + size]) <= set("ACGT"):
            return o
    raise AssertionError("no clean stretch")


def hand_cases():
    """[(name, cigar, seq, chrom, pos, MD, cs)]; MD and cs written out from the letters of the reference, or None: the independent
    writer alone says what they are"""
    R = CHROMS[0]
    o = clean_window(R, 1200)
    p = o + 1

    def with_mis(n, at):
        s = list(R[o:o + n])
        for k in at:
            s[k] = mut(R[o + k])
        return "".join(s)
    c = [("insertion does not reset MD", "10M2I10M", R[o:o + 10] + "ac" + R[o + 10:o + 20], 0, p, "20", ":10+ac:10"),
         ("two mismatches in a row", "10M", with_mis(10, (4, 5)), 0, p, "4%s0%s4" % (R[o + 4], R[o + 5]),
          ":4*%s%s*%s%s:4" % (R[o + 4].lower(), mut(R[o + 4]).lower(), R[o + 5].lower(), mut(R[o + 5]).lower())),
         ("mismatch behind a deletion", "5M2D5M", R[o:o + 5] + mut(R[o + 7]) + R[o + 8:o + 12], 0, p, "5^%s0%s4" % (R[o + 5:o + 7], R[o + 7]),
          ":5-%s*%s%s:4" % (R[o + 5:o + 7].lower(), R[o + 7].lower(), mut(R[o + 7]).lower())),
         ("two D ops in a row", "5M2D1D5M", R[o:o + 5] + R[o + 8:o + 13], 0, p, "5^%s0^%s5" % (R[o + 5:o + 7], R[o + 7]),
          ":5-%s-%s:5" % (R[o + 5:o + 7].lower(), R[o + 7].lower())),
         ("D, I, D between two columns", "5M1D2I1D5M", R[o:o + 5] + "gg" + R[o + 7:o + 12], 0, p, "5^%s0^%s5" % (R[o + 5], R[o + 6]),
          ":5-%s+gg-%s:5" % (R[o + 5].lower(), R[o + 6].lower())),
         ("mismatch in front of and behind an I", "5M1I5M", with_mis(5, (4,)) + "t" + mut(R[o + 5]) + R[o + 6:o + 10], 0, p,
          "4%s0%s4" % (R[o + 4], R[o + 5]), ":4*%s%s+t*%s%s:4" % (R[o + 4].lower(), mut(R[o + 4]).lower(), R[o + 5].lower(), mut(R[o + 5]).lower())),
         ("mismatch in front of and behind a D", "5M1D5M", with_mis(5, (4,)) + mut(R[o + 6]) + R[o + 7:o + 11], 0, p,
          "4%s0^%s0%s4" % (R[o + 4], R[o + 5], R[o + 6]),
          ":4*%s%s-%s*%s%s:4" % (R[o + 4].lower(), mut(R[o + 4]).lower(), R[o + 5].lower(), R[o + 6].lower(), mut(R[o + 6]).lower())),
         ("a run across M, = and X", "5M5=5X", R[o:o + 15], 0, p, "15", ":15"),
         ("X on matching bases, = on a mismatch", "3X1=3X", with_mis(7, (3,)), 0, p, "3%s3" % R[o + 3], ":3*%s%s:3" % (R[o + 3].lower(), mut(R[o + 3]).lower())),
         ("clips of both kinds at both ends", "2H3S10M4S1H", "ttt" + R[o:o + 10] + "gggg", 0, p, "10", ":10"),
         ("lower-case SEQ", "10M", R[o:o + 10].lower(), 0, p, "10", ":10"),
         ("lower-case mismatch and insertion", "3M2I3M", (R[o:o + 2] + mut(R[o + 2]) + "CA" + R[o + 3:o + 6]).lower(), 0, p, "2%s3" % R[o + 2],
          ":2*%s%s+ca:3" % (R[o + 2].lower(), mut(R[o + 2]).lower())),
         ("leading D, trailing I", "2D5M1I", R[o + 2:o + 7] + "t", 0, p, "0^%s5" % R[o:o + 2], "-%s:5+t" % R[o:o + 2].lower()),
         ("trailing D", "5M2D", R[o:o + 5], 0, p, "5^%s0" % R[o + 5:o + 7], ":5-%s" % R[o + 5:o + 7].lower()),
         ("leading I", "2I5M", "gg" + R[o:o + 5], 0, p, "5", "+gg:5"),
         ("one column, a match", "1M", R[o], 0, p, "1", ":1"),
         ("one column, a mismatch", "1M", mut(R[o]), 0, p, "0%s0" % R[o], "*%s%s" % (R[o].lower(), mut(R[o]).lower())),
         ("mismatch in column 0 and in the last", "20M", with_mis(20, (0, 19)), 0, p, "0%s18%s0" % (R[o], R[o + 19]),
          "*%s%s:18*%s%s" % (R[o].lower(), mut(R[o]).lower(), R[o + 19].lower(), mut(R[o + 19]).lower())),
         ("mismatch in lane 0 and in lane 63 of a step", "200M", with_mis(200, (64, 127)), 0, p, "64%s62%s72" % (R[o + 64], R[o + 127]),
          ":64*%s%s:62*%s%s:72" % (R[o + 64].lower(), mut(R[o + 64]).lower(), R[o + 127].lower(), mut(R[o + 127]).lower())),
         ("mismatches on both sides of a step boundary", "130M", with_mis(130, (63, 64)), 0, p, "63%s0%s65" % (R[o + 63], R[o + 64]),
          ":63*%s%s*%s%s:65" % (R[o + 63].lower(), mut(R[o + 63]).lower(), R[o + 64].lower(), mut(R[o + 64]).lower())),
         ("a deletion on a step boundary", "64M3D64M", R[o:o + 64] + R[o + 67:o + 131], 0, p, "64^%s64" % R[o + 64:o + 67], ":64-%s:64" % R[o + 64:o + 67].lower()),
         ("an insertion on a step boundary", "128M3I10M", R[o:o + 128] + "acg" + R[o + 128:o + 138], 0, p, "138", ":128+acg:10")]
    for n in (63, 64, 65, 127, 128, 129, 9, 10, 99, 100, 999, 1000):
        c.append(("a run of %d" % n, "%dM" % n, R[o:o + n], 0, p, "%d" % n, ":%d" % n))
        c.append(("a run of %d and a mismatch" % n, "%dM" % (n + 1), with_mis(n + 1, (n,)), 0, p, "%d%s0" % (n, R[o + n]),
                  ":%d*%s%s" % (n, R[o + n].lower(), mut(R[o + n]).lower())))
        c.append(("a run of %d, an insertion, a run of %d" % (n, n), "%dM1I%dM" % (n, n), R[o:o + n] + "a" + R[o + n:o + 2 * n], 0, p, "%d" % (2 * n),
                  ":%d+a:%d" % (n, n)))
    # N: in the reference, in SEQ, in both
    nz = next(i for i in range(2, len(R)) if R[i] == "N" and "N" not in R[i - 2:i])
    c += [("N in the reference", "3M", R[nz - 2:nz] + "A", 0, nz - 1, "2N0", ":2*na"),
          ("N in both", "3M", R[nz - 2:nz] + "N", 0, nz - 1, "2N0", ":2*nn"),
          ("n in both", "3M", R[nz - 2:nz] + "n", 0, nz - 1, "2N0", ":2*nn"),
          ("N in SEQ", "5M", R[o] + "N" + R[o + 2:o + 5], 0, p, "1%s3" % R[o + 1], ":1*%sn:3" % R[o + 1].lower())]
    # an ambiguity code in both is a match (the letters are equal), in one of them a mismatch
    code, at = next((R[i], i) for i in range(2, len(R)) if R[i] in "YRWSKMDVHB" and set(R[i - 2:i]) <= set("ACGT"))
    c += [("the same code in both", "3M", R[at - 2:at + 1], 0, at - 1, "3", ":3"),
          ("a code in the reference", "3M", R[at - 2:at] + "A", 0, at - 1, "2%s0" % code, ":2*%sa" % code.lower())]
    # the first base of a chromosome, the last base of the last chromosome, the same read on two chromosomes
    last = CHROMS[2]
    c += [("POS 1", "30M", R[:30], 0, 1, None, None),
          ("ends on the last base of the last chromosome", "3S40M", "acg" + last[-40:], 2, len(last) - 39, None, None),
          ("ends there with a deletion", "20M5D", last[-25:-5], 2, len(last) - 24, None, None),
          ("on chromosome 0", "30M", R[o:o + 30], 0, p, "30", ":30"),
          ("the same on chromosome 2", "30M", R[o:o + 30], 2, p, None, None),
          ("the same on chromosome 1", "30M", R[o:o + 30], 1, p, None, None)]
    return c


def check_hand_cases(eng):
    cases = hand_cases()
    got = tags(eng, [(c[1], c[2], c[3], c[4]) for c in cases])
    for c, g in zip(cases, got):
        want = write_tags(c[1], c[4], c[2], CHROMS[c[3]])
        assert g == want, c[0]
        if c[5] is not None:
            assert g == (c[5], c[6]), c[0]
    for c, g in list(zip(cases, got))[::7]:                          # ... and alone
        assert tags(eng, [(c[1], c[2], c[3], c[4])]) == [g], c[0]
    r = characterize.cs_md_call(eng, [], [], [], [])                 # n == 0
    assert (r["md"], r["cs"], r["md_off"].tolist(), r["cs_off"].tolist()) == (b"", b"", [0], [0])
    return got


def test_host_hand_written_cases(host):
    got = check_hand_cases(host)
    assert len(got) > 60


# ---- seeded random records ------------------------------------------------------------------------------------------------------------
_RANDOM = {}


def random_records():
    """the 2 000 generated records and what the independent writer says of them, made once"""
    if not _RANDOM:
        recs = calmd_lib.random_records()
        _RANDOM["records"] = recs
        _RANDOM["writer"] = [write_tags(r["cigar"], r["pos"], r["seq"], CHROMS[r["chrom"]]) for r in recs]
        _RANDOM["writer_eqx"] = [write_tags(r["cigar_eqx"], r["pos"], r["seq"], CHROMS[r["chrom"]]) for r in recs[:300]]
    return _RANDOM


def check_random_records(eng):
    fx = random_records()
    recs = fx["records"]
    assert len(recs) == 2000 and max(len(r["seq"]) for r in recs) > 2500 and any(r["cigar"].endswith("1M") and len(r["md"]) <= 3 for r in recs)
    truth = [(r["md"], r["cs"]) for r in recs]
    assert fx["writer"] == truth and fx["writer_eqx"] == truth[:300]
    got = tags(eng, [(r["cigar"], r["seq"], r["chrom"], r["pos"]) for r in recs])
    for r, g, t in zip(recs, got, truth):
        assert g == t, r["name"]
    got = tags(eng, [(r["cigar_eqx"], r["seq"], r["chrom"], r["pos"]) for r in recs[:300]])
    assert got == truth[:300]


def test_host_random_records_three_ways(host):
    check_random_records(host)


def test_new_md_gives_the_reference_line_through_the_existing_line_pairs(host):
    """pairs_from_sam (the existing host build of ns_sam_pairs.h) on (CIGAR, the new MD, SEQ): its reference line is the slice of the
    reference with `-` where the read inserts"""
    from tests.test_sam_pairs import build_host_walk
    walk = build_host_walk()
    recs = [r for r in random_records()["records"] if "H" not in r["cigar"]][:200]
    got = tags(host, [(r["cigar"], r["seq"], r["chrom"], r["pos"]) for r in recs])
    sam = [(r["name"], r["flag"], REF.names[r["chrom"]], r["pos"], r["cigar"], md, r["seq"]) for r, (md, _) in zip(recs, got)]
    sam += [(r["name"], r["flag"], REF.names[r["chrom"]], r["pos"], r["cigar_eqx"], md, r["seq"]) for r, (md, _) in zip(recs[:100], got)]
    packed = characterize.pairs_from_sam(walk, sam)
    assert len(packed) == len(sam) == 300
    for i, s in enumerate(sam):
        at, want = s[3] - 1, []
        chrom = CHROMS[REF.names.index(s[2])]
        for n, op in re.findall(r"(\d+)([MIDSH=X])", s[4]):
            n = int(n)
            if op in "M=XD":
                want.append(chrom[at:at + n])
                at += n
            elif op == "I":
                want.append("-" * n)
        assert packed[i][2].upper() == "".join(want), s[0]


# ---- bad records ------------------------------------------------------------------------------------------------------------------------
def bad_cases():
    """[(name, cigar, seq, chrom, pos, reason)]"""
    R, last = CHROMS[0], CHROMS[2]
    o = clean_window(R, 100)
    p = o + 1
    s5, s40 = R[o:o + 5], R[o:o + 40]
    return [("digits at the end", "5M3", s5, 0, p, 1), ("no count", "M5", s5, 0, p, 1), ("a star", "*", s5, 0, p, 1), ("empty", "", s5, 0, p, 1),
            ("a count of 0", "5M0I", s5, 0, p, 1), ("a comma", "3M,2M", s5, 0, p, 1), ("ten digits", "0000000005M", s5, 0, p, 1),
            ("2^28", "268435456M", s5, 0, p, 1), ("a count of 0 behind a round", "40M0D", s40, 0, p, 1),
            ("N", "2M3N3M", s5, 0, p, 2), ("P", "5M2P", s5, 0, p, 2), ("a lower-case op", "5m", s5, 0, p, 2), ("B", "5B", s5, 0, p, 2),
            ("S between columns", "2M1S2M", s5, 0, p, 3), ("two leading S", "1S1S3M", s5, 0, p, 3), ("two trailing S", "3M1S1S", s5, 0, p, 3),
            ("H inside S", "1S2H4M", s5, 0, p, 3), ("S behind the last H", "4M2H1S", s5, 0, p, 3), ("H between columns", "2M2H3M", s5, 0, p, 3),
            ("three H", "1H1H5M", s5, 0, p, 3),
            ("SEQ too long", "4M", s5, 0, p, 4), ("SEQ too short", "3S5M", s5, 0, p, 4), ("SEQ empty", "5M", "", 0, p, 4), ("H counted", "5M", s5[:4], 0, p, 4),
            ("a star in SEQ", "5M", s5[:2] + "*" + s5[3:], 0, p, 5), ("a digit in a clip", "2S3M", "1" + s5[1:], 0, p, 5),
            ("= in SEQ", "40M", s40[:20] + "=" + s40[21:], 0, p, 5), ("a bracket in the last byte", "40M", s40[:39] + "[", 0, p, 5),
            ("a grave in an insertion", "20M1I19M", s40[:20] + "`" + s40[21:], 0, p, 5), ("a byte above 127", "5M", s5[:4] + "é", 0, p, 5),
            ("chrom == nchrom", "5M", s5, 3, p, 6), ("chrom 2^32 - 1", "5M", s5, 2 ** 32 - 1, p, 6),
            ("POS 0", "5M", s5, 0, 0, 7),
            ("one base past the end", "5M", s5, 2, len(last) - 3, 8), ("past the end of chromosome 0, into chromosome 1", "5M", s5, 0, len(R) - 3, 8),
            ("a deletion past the end", "2M10D3M", s5, 2, len(last) - 10, 8), ("POS behind the end", "5M", s5, 1, len(CHROMS[1]) + 1, 8),
            ("POS 2^32 - 1", "5M", s5, 0, 2 ** 32 - 1, 8),
            ("clips only", "5S", s5, 0, p, 9), ("an insertion only", "5I", s5, 0, p, 9), ("a deletion only", "5D", "", 0, p, 9), ("H only", "3H", "", 0, p, 9)]


def seq_bytes(s):
    return s.encode("latin-1")


def check_bad_records(eng):
    cases = bad_cases()
    assert set(c[5] for c in cases) == set(range(1, 10)) == set(characterize.CALMD_BAD_REASONS)
    R = CHROMS[0]
    o = clean_window(R, 100)
    good = ("10M", R[o:o + 10], 0, o + 1)
    for name, cigar, seq, chrom, pos, reason in cases:
        r = characterize.calmd_raw(eng, [good[0], cigar, good[0]], [good[1], seq_bytes(seq), good[1]], [0, chrom, 0], [good[3], pos, good[3]])
        assert (r["n_bad"], r["first_bad"], r["bad_reason"]) == (1, 1, reason), name
        assert (r["md"], r["cs"], r["md_off"].tolist(), r["cs_off"].tolist()) == (b"1010", b":10:10", [0, 2, 2, 4], [0, 3, 3, 6]), name
        with pytest.raises(ValueError, match="the first is record 1 ") as e:
            characterize.cs_md_call(eng, [good[0], cigar, good[0]], [good[1], seq_bytes(seq), good[1]], [0, chrom, 0], [good[3], pos, good[3]])
        assert characterize.CALMD_BAD_REASONS[reason] in str(e.value), name
    # all of them in one call, the first one first; and a good call afterwards
    r = characterize.calmd_raw(eng, [c[1] for c in cases], [seq_bytes(c[2]) for c in cases], [c[3] for c in cases], [c[4] for c in cases])
    assert (r["n_bad"], r["first_bad"], r["bad_reason"], r["md"], r["cs"]) == (len(cases), 0, 1, b"", b"")
    assert tags(eng, [good]) == [("10", ":10")]


def test_host_bad_records(host):
    check_bad_records(host)


# ---- the cross-lane arithmetic: what one lane cannot show (run on the one-lane build, on 64 lanes in lock step and on the GPU) ------------
def built(ops, o, mis=(), chrom=0):
    """(cigar, seq, chrom, pos) of the ops [(count, letter)] laid on chromosome `chrom` from offset o: the reference's letters in the
    columns, but for the columns `mis`; `acgt...` in lower case for I and S"""
    R = CHROMS[chrom]
    r, col, seq = o, 0, []
    for n, op in ops:
        if op in "M=X":
            seq.append("".join(mut(R[r + k]) if col + k in mis else R[r + k] for k in range(n)))
            r += n
            col += n
        elif op == "D":
            r += n
        elif op in "IS":
            seq.append(("acgt" * (n // 4 + 1))[:n])
    return "".join("%d%s" % x for x in ops), "".join(seq), chrom, o + 1


def ops_of(text):
    return [(int(n), op) for n, op in re.findall(r"(\d+)([MIDSH=X])", text)]


PAIRS15 = "1M1I" * 15                                                  # 60 bytes, 30 ops
TAILS = {3: "10M", 4: "1M1D", 5: "10M1M", 6: "10M10M", 7: "10M1D1M", 8: "1M1D1M1D"}


def cigar_of_length(n, shift=False):
    """a dense good CIGAR of exactly n bytes; shift: with `10M` in front, so that its op letters stand at the other bytes"""
    head = "10M" if shift else ""
    pairs = (n - len(head) - 3) // 4
    text = head + "1M1I" * pairs
    return text + TAILS[n - len(text)]


def wave_cases():
    """[(name, cigar, seq, chrom, pos, reason or None)] — reason: written out where it can be counted by hand, 0 for a good record; None:
    calmd_lib.bad_reason alone says.  The texts of the good ones are the independent writer's."""
    R, last = CHROMS[0], CHROMS[2]
    o = clean_window(R, 1200)
    p = o + 1
    c = []

    def good(name, text, mis=()):
        c.append((name,) + built(ops_of(text), o, mis) + (0,))
    # ---- calmd_ops: rounds of 64 CIGAR bytes
    for n in (63, 64, 65, 127, 128, 129):
        for shift in (False, True):
            text = cigar_of_length(n, shift)
            assert len(text) == n
            good("a CIGAR of %d bytes%s" % (n, ", shifted" if shift else ""), text)
    a, b = PAIRS15 + "1M2D", PAIRS15 + "10M2D"
    assert a[63] == "D" and b[64] == "D"
    good("an op letter at byte 63", a + "5M")
    good("an op letter at byte 64", b + "5M")
    straddle = PAIRS15 + "2M123D5M"
    assert straddle[62:66] == "123D"
    good("a count across the boundary of a round", straddle)
    s5 = R[o:o + 5]
    big = 268435455                                                  # 2^28 - 1: eight of them are 2^31 - 8
    c += [("nine digits, valid, a deletion past the end", "5M100000000D", s5, 0, p, 8),
          ("nine digits, valid, SEQ too short", "100000000M", s5, 0, p, 4),
          ("nine digits with zeros in front", "000000005M", s5, 0, p, 0),
          ("SEQ bytes 2^31 - 1", "1M" + ("%dI" % big) * 8 + "6I", "A", 0, p, 4),
          ("SEQ bytes 2^31", "1M" + ("%dI" % big) * 8 + "7I", "A", 0, p, 1),
          ("SEQ bytes 2^31 in clips", "%dS" % big + ("%dI" % big) * 7 + "8S1M", "A", 0, p, 1),
          ("reference letters 2^31 - 1", "1M" + ("%dD" % big) * 8 + "6D", R[o], 0, p, 8),
          ("reference letters 2^31", "1M" + ("%dD" % big) * 8 + "7D", R[o], 0, p, 1),
          ("columns 2^31 - 1", ("%dM" % big) * 8 + "7M", s5, 0, p, 4),
          ("columns 2^31", ("%dM" % big) * 8 + "8M", s5, 0, p, 1),
          ("columns 2^31 in = and X", ("%d=" % big) * 4 + ("%dX" % big) * 4 + "8=", s5, 0, p, 1)]
    # the order of the clips, the clip in one round and the op that offends in the next (62 bytes in front)
    lead = PAIRS15 + "1M"
    for name, text in (("H between columns", lead + "2H3M"), ("an op behind a trailing S", lead + "2S3M"), ("two trailing S", lead + "2S1S"),
                       ("an I behind a trailing S", lead + "2S1I"), ("S behind the closing H", lead + "2H1S"), ("H behind the closing H", lead + "2H1H")):
        assert len(text) == 66 and text[63] in "HS"                  # (the clip closes round 0, the op that offends stands at bytes 64 and 65)
        cg, sq, _, _ = built(ops_of(text), o)
        c.append((name + " across a round", cg, sq, 0, p, 3))
    good("S and a closing H across a round", lead + "2S3H")
    good("leading H and S, the first column in a later round", "2H3S" + "1I1D" * 16 + "5M")
    good("leading S, the first column in the third round", "3S" + "1D1I" * 32 + "5M2S1H")
    c += [("two errors in one round, the op first", "5M2N3M0I", s5 + R[o + 5:o + 8], 0, p, 2),
          ("two errors in one round, the count first", "5M0I2N3M", s5 + R[o + 5:o + 8], 0, p, 1),
          ("a clip error in front of an unknown op", "2M1S1S2N", s5, 0, p, 3),
          ("an unknown op behind a trailing S", "2M1S2N1S", s5, 0, p, 2),
          ("an unknown op in front of a clip error", "2M2N1S2M", s5, 0, p, 2),
          ("an unknown op in the first round, a parse error in the second", PAIRS15 + "1M2N" + "0M", s5, 0, p, 2),
          ("a parse error in the second round only", PAIRS15 + "1M2M" + "0M", s5, 0, p, 1),
          ("digits at the end behind a round", PAIRS15 + "1M2M" + "5", s5, 0, p, 1)]
    # the densest op table there is, odd and even lengths next to each other (the tables lie at calmd_op_base)
    for text in ("1M1I" * 64, "10M" + "1I1M" * 62, "10M" + "1D1M" * 62, "1M1D" * 64, "10M", "1M1I" * 64, "1M", "10M" + "1I1M" * 62):
        good("dense, %d bytes" % len(text), text)
    c += [("a good record in front of one that begins with a letter", "10M", R[o:o + 10], 0, p, 0), ("a letter first", "M5", s5, 0, p, 1),
          ("a good record whose CIGAR fills its round, in front of a letter", cigar_of_length(64)) + built(ops_of(cigar_of_length(64)), o)[1:] + (0,),
          ("a letter first, again", "M5", s5, 0, p, 1), ("a good record in front of an op", "7M", R[o:o + 7], 0, p, 0), ("the op", "5M", s5, 0, p, 0)]
    # ---- calmd_text: steps of 64 columns
    for n in (64, 128):
        good("a trailing D behind %d columns" % n, "%dM2D" % n)
        good("a trailing I behind %d columns" % n, "%dM2I" % n)
        good("a trailing D and I behind %d columns" % n, "%dM2D1I" % n)
        good("a trailing I and D behind %d columns, a mismatch in the last" % n, "%dM1I2D" % n, (n - 1,))
    good("a mismatch in lane 63, a D in front of lane 0", "64M2D10M", (63,))
    good("a mismatch in lane 63, an I in front of lane 0", "64M2I10M", (63,))
    good("a mismatch in lane 63 and in lane 0, a D between", "64M1D10M", (63, 64))
    good("D, I, D on a step boundary", "64M1D2I1D10M")
    good("D, I, D on the second step boundary, mismatches around", "128M1D2I1D10M", (127, 128))
    good("64 one-column ops in one step, a long op behind", "1M1D" * 64 + "100M", (70, 127, 128))
    good("a step that begins in the middle of a long op", "1M1I" * 32 + "200M", (31, 32, 63, 64, 191))
    good("one-column ops behind a long op", "100M" + "1D1M" * 70, (99, 100, 128))
    for n in (64, 65, 300):
        good("an insertion of %d" % n, "10M%dI10M" % n)
        good("a deletion of %d" % n, "10M%dD10M" % n, (9, 10))
        good("an insertion and a deletion of %d on a step boundary" % n, "64M%dI%dD64M" % (n, n))
    # ---- calmd_seq_letters: 8 bytes per lane, 512 per round
    for sn in (512, 513, 519):
        for at in sorted(set((0, 7, 8, 511, 512, sn - 1))):
            if at < sn:
                sq = R[o:o + at] + "@[`{1*"[at % 6] + R[o + at + 1:o + sn]
                c.append(("a bad SEQ byte at %d of %d" % (at, sn), "%dM" % sn, sq, 0, p, 5))
        good("%d letters" % sn, "%dM" % sn, (sn - 1,))
    return c


def check_wave_cases(eng):
    """the cases of wave_cases in one call, the bad ones among the good: every reason, the first bad record, the texts of the good ones"""
    cases = wave_cases()
    want = []
    for name, cigar, seq, chrom, pos, reason in cases:
        ref = calmd_lib.bad_reason(cigar, seq, chrom, pos, CHROMS)
        assert reason is None or reason == ref, name
        want.append(ref)
    assert set(want) >= {0, 1, 2, 3, 4, 5, 8}
    r = characterize.calmd_raw(eng, [c[1] for c in cases], [seq_bytes(c[2]) for c in cases], [c[3] for c in cases], [c[4] for c in cases])
    md, cs = characterize.texts_of(r, "md"), characterize.texts_of(r, "cs")
    first = next(i for i, w in enumerate(want) if w)
    for i, (c, w) in enumerate(zip(cases, want)):
        assert (md[i], cs[i]) == (("", "") if w else write_tags(c[1], c[4], c[2], CHROMS[c[3]])), c[0]
        alone = characterize.calmd_raw(eng, [c[1]], [seq_bytes(c[2])], [c[3]], [c[4]])
        assert (alone["n_bad"], alone["bad_reason"]) == ((1, w) if w else (0, 0)), c[0]
        assert (alone["md"].decode(), alone["cs"].decode()) == (md[i], cs[i]), c[0]
    assert (r["n_bad"], r["first_bad"], r["bad_reason"]) == (sum(1 for w in want if w), first, want[first])
    return len(cases)


def check_neighbours(eng):
    """a good record between two records whose CIGARs begin with a letter, an op letter behind a count, `=` or digits: the lane behind the
    last byte of a CIGAR, and the one in front of the first, take nothing of the neighbour"""
    R = CHROMS[0]
    o = clean_window(R, 1200)
    for cigar in ("1M", "10M", cigar_of_length(63), cigar_of_length(64), cigar_of_length(65), cigar_of_length(128)):
        rec = built(ops_of(cigar), o)
        want = write_tags(rec[0], rec[3], rec[1], R)
        for behind, reason in (("M5", 1), ("5M", 0), ("=", 1), ("15", 1), ("N", 1)):
            got = characterize.calmd_raw(eng, [behind, rec[0], behind, rec[0]], [R[o:o + 5], rec[1], R[o:o + 5], rec[1]], [0] * 4, [o + 1] * 4)
            texts = list(zip(characterize.texts_of(got, "md"), characterize.texts_of(got, "cs")))
            assert texts[1] == texts[3] == want, (cigar, behind)
            assert texts[0] == texts[2] == (("", "") if reason else ("5", ":5")), (cigar, behind)
            assert (got["n_bad"], got["bad_reason"]) == ((2, reason) if reason else (0, 0)), (cigar, behind)


def check_store_guard(host):
    """the host build alone (the engine has no such entry): calmd_text<true> on room one byte shorter and one byte longer than
    measured, for MD and for cs, says so and stores nothing outside — on records whose last store is a run, a mismatch, a deletion, an
    insertion, and in a later step"""
    cases = [c for c in hand_cases()[:24]] + [c for c in wave_cases() if c[5] == 0][::6]
    assert len(cases) > 30
    for c in cases:
        cg, sq = c[1].encode(), seq_bytes(c[2])
        assert host.guard(cg, len(cg), sq, len(sq), c[3], c[4]) == 0, c[0]
    assert host.guard(b"M5", 2, b"ACGTA", 5, 0, 1) == 1


def test_host_store_guard(host):
    check_store_guard(host)


def test_host_cross_lane_cases(host):
    assert check_wave_cases(host) > 90
    check_neighbours(host)


_CORRUPTED = {}


def corrupted_records():
    """the generated corrupted set with what the references say of it, made once: bad_reason for all of them (checked against the 42
    literal reasons of bad_cases first), write_tags for those that stayed good"""
    if not _CORRUPTED:
        for c in bad_cases():
            assert calmd_lib.bad_reason(c[1], c[2], c[3], c[4], CHROMS) == c[5], c[0]
        recs = calmd_lib.corrupted_records()
        _CORRUPTED["records"] = recs
        _CORRUPTED["texts"] = [("", "") if r["reason"] else write_tags(r["cigar"], r["pos"], r["seq"].decode("latin-1"), CHROMS[r["chrom"]]) for r in recs]
    return _CORRUPTED


def check_corrupted_records(eng, alone: int = 1):
    """all of them in one call (the texts of those that stayed good, the count of the bad ones, the first), and every `alone`-th record
    in a call of its own (its reason)"""
    fx = corrupted_records()
    recs, texts = fx["records"], fx["texts"]
    assert len(recs) == 3000 and set(r["reason"] for r in recs) == set(range(10))
    assert sum(1 for r in recs if r["two"]) >= 200                    # two errors in one CIGAR, of different reasons at different bytes
    assert sum(1 for r in recs if r["reason"] in (1, 2, 3) and r["at"] >= LANES) >= 200
    got = characterize.calmd_raw(eng, [r["cigar"] for r in recs], [r["seq"] for r in recs], [r["chrom"] for r in recs], [r["pos"] for r in recs])
    first = next(i for i, r in enumerate(recs) if r["reason"])
    assert (got["n_bad"], got["first_bad"], got["bad_reason"]) == (sum(1 for r in recs if r["reason"]), first, recs[first]["reason"])
    assert list(zip(characterize.texts_of(got, "md"), characterize.texts_of(got, "cs"))) == texts
    for r in recs[::alone]:
        one = characterize.calmd_raw(eng, [r["cigar"]], [r["seq"]], [r["chrom"]], [r["pos"]])
        assert (one["n_bad"], one["bad_reason"]) == ((1, r["reason"]) if r["reason"] else (0, 0)), (r["cigar"], r["chrom"], r["pos"])
    return fx


def test_host_corrupted_records(host):
    check_corrupted_records(host)


def checksum(md, md_off, cs, cs_off):
    s = 0
    for part in (md, md_off, cs, cs_off):
        for c in part:
            s = (s * 31 + int(c)) & (2 ** 64 - 1)
    return s


def test_host_code_is_clean_under_the_sanitizers(host, tmp_path):
    """the walks as a stand-alone program under -fsanitize=address,undefined, every record on copies of exactly its size (CIGAR, SEQ,
    op table, texts, and only the chromosome it lies on): the bad records give their reasons and read nothing outside, the good ones
    their texts (the checksum of texts and offsets)"""
    out = os.path.join(ROOT, "tests", "_tmp")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "calmd_host_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DCALMD_HOST_MAIN", "-o", exe,
                           os.path.join(ROOT, "tests", "calmd_host.cpp")])
    genome = "".join("C %s\n" % REF.chrom(i).tobytes().decode("latin-1") for i in range(3))

    def run(records):
        p = os.path.join(str(tmp_path), "records.txt")
        with open(p, "w", encoding="latin-1") as f:
            f.write(genome + "".join("R %s %s %d %d\n" % (c or "~", s or "~", ch, ps) for c, s, ch, ps in records))
        a, b = subprocess.check_output([exe, p], text=True).strip().split("\n")
        return [int(x) for x in a.split()], int(b)
    R = CHROMS[0]
    o = clean_window(R, 100)
    good = ("10M", R[o:o + 10], 0, o + 1)
    for name, cigar, seq, chrom, pos, reason in bad_cases():
        assert run([good, (cigar, seq, chrom, pos), good]) == ([3, 1, 1, reason], checksum(b"1010", [0, 2, 2, 4], b":10:10", [0, 3, 3, 6])), name
    cases = hand_cases()
    recs = [(c[1], c[2], c[3], c[4]) for c in cases] + [(r["cigar"], r["seq"], r["chrom"], r["pos"]) for r in random_records()["records"][:300]]
    want = characterize.calmd_raw(host, [r[0] for r in recs], [r[1] for r in recs], [r[2] for r in recs], [r[3] for r in recs])
    assert want["n_bad"] == 0
    assert run(recs) == ([len(recs), 0, -1, 0], checksum(want["md"], want["md_off"].tolist(), want["cs"], want["cs_off"].tolist()))
    assert run([]) == ([0, 0, -1, 0], checksum(b"", [0], b"", [0]))


def test_host_argument_checks(host):
    cg, cg_off = characterize._pack(["5M", "5M"])
    sq, sq_off = characterize._pack(["ACGTA", "ACGTA"])
    ch, ps = np.zeros(2, dtype=np.uint32), np.ones(2, dtype=np.uint32)
    out = characterize.NsCalmdResult()

    def call(*a):
        return host.L.ns_calmd(None, *[x.ctypes.data if x is not None else None for x in a], 2, C.addressof(out))
    assert call(cg, cg_off, sq, sq_off, ch, ps) == 0 and out.n_bad == 0
    for args in ((cg, None, sq, sq_off, ch, ps), (cg, cg_off, sq, sq_off, None, ps), (cg, cg_off, sq, sq_off, ch, None), (None, cg_off, sq, sq_off, ch, ps),
                 (cg, cg_off[::-1].copy(), sq, sq_off, ch, ps), (cg, cg_off, sq, (sq_off + 1).astype(np.uint64), ch, ps)):
        assert call(*args) == -1


# ---- the Python side on the stand-in engine -------------------------------------------------------------------------------------------
def mixed_sam_text():
    """records with both tags, with one, with none; unmapped ones, one without SEQ, a short line; a header line between records"""
    recs = [r for r in calmd_lib.random_records(seed=11, n=40, max_cols=300)]
    both = calmd_lib.sam_text(recs, REF).splitlines(True)
    header, lines = [x for x in both if x.startswith("@")], [x for x in both if not x.startswith("@")]
    out = list(header)
    for i, line in enumerate(lines):
        f = line.rstrip("\n").split("\t")
        if i % 4 == 1:
            f = [t for t in f if not t.startswith("MD:Z:")]
        elif i % 4 == 2:
            f = [t for t in f if not t.startswith("cs:Z:")]
        elif i % 4 == 3:
            f = [t for t in f if not t.startswith(("cs:Z:", "MD:Z:"))] + ["zz:Z:last"]
        out.append("\t".join(f) + "\n")
        if i == 7:
            out += ["un1\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\tIIII\n", "un2\t4\t%s\t5\t0\t4M\t*\t0\t0\tACGT\tIIII\n" % REF.names[0],
                    "noseq\t256\t%s\t5\t0\t4M\t*\t0\t0\t*\t*\n" % REF.names[1], "nocigar\t0\t%s\t5\t0\t*\t*\t0\t0\tACGT\tIIII\n" % REF.names[1],
                    "norname\t0\t*\t5\t0\t4M\t*\t0\t0\tACGT\tIIII\n", "short\t0\t%s\t5\t0\t4M\n" % REF.names[0], "@CO\ta comment between records\n"]
    return "".join(out)


def check_tagged_text(eng, tmp_path):
    text = mixed_sam_text()
    want = calmd_lib.retagged(text, REF)
    assert want != text and calmd_lib.strip_tags(want) == calmd_lib.strip_tags(text)
    path = os.path.join(str(tmp_path), "mixed.sam")
    with open(path, "w") as f:
        f.write(text)
    tagged = characterize.with_reference(path, calmd_lib.GENOME, eng)
    assert isinstance(tagged, characterize.SamSource) and str(tagged) == path
    got = "".join(tagged)
    assert got == want == "".join(tagged)                            # (re-iterable)
    n_rec = sum(1 for x in text.splitlines() if not x.startswith("@"))
    n_tag = sum(1 for a, b in zip(text.splitlines(), want.splitlines()) if a != b)
    assert (tagged.n_records, tagged.n_tagged) == (n_rec, n_tag) and 0 < n_tag < n_rec
    for a, b in zip(text.splitlines(True), got.splitlines(True)):   # appended only: every other byte stands
        assert b.startswith(a.rstrip("\n")) and (a == b or "\tMD:Z:" in b[len(a) - 1:] or "\tcs:Z:" in b[len(a) - 1:])
        if a.startswith(("un", "noseq", "nocigar", "norname", "short", "@")):
            assert a == b
    for batch in (1, 200, 1000):                                     # batches cut at every record, and at some
        assert "".join(characterize.with_reference(path, REF, eng, batch_bytes=batch)) == want
    out = os.path.join(str(tmp_path), "tagged.sam")
    assert characterize.calmd(path, REF, out, eng) == (n_rec, n_tag) and open(out).read() == want
    # the readers over it: what they give on the text with the independent writer's tags
    with open(out, "w") as f:
        f.write(want)
    stripped = os.path.join(str(tmp_path), "stripped.sam")
    bare = "".join(x for x in calmd_lib.strip_tags(text).splitlines(True) if not x.startswith(("un2", "noseq", "norname")))    # (pass through with a CIGAR: cs_from_sam wants a tag of them)
    with open(stripped, "w") as f:
        f.write(bare)
    again = characterize.with_reference(stripped, REF, eng)
    full = os.path.join(str(tmp_path), "full.sam")
    with open(full, "w") as f:
        f.write(calmd_lib.retagged(bare, REF))
    assert characterize.cs_from_sam(again) == characterize.cs_from_sam(full)
    with pytest.raises(ValueError, match="neither a cs nor an MD tag"):
        characterize.cs_from_sam(stripped)
    # a file without a newline at its end
    with open(path, "w") as f:
        f.write(calmd_lib.strip_tags(text).rstrip("\n"))
    assert "".join(characterize.with_reference(path, REF, eng)) == calmd_lib.retagged(calmd_lib.strip_tags(text), REF).rstrip("\n")
    return want


def test_tagged_text_on_the_host(host, tmp_path):
    check_tagged_text(host, tmp_path)


def test_tagged_text_over_bam_text(host, tmp_path):
    from tests.test_bam import build_host as build_bam_host
    text = calmd_lib.strip_tags(calmd_lib.sam_text(calmd_lib.random_records(seed=12, n=30, max_cols=200), REF))
    path = os.path.join(str(tmp_path), "stripped.bam")
    with open(path, "wb") as f:
        f.write(bam_lib.sam_to_bam(text))
    bam = characterize.read_bam(path, build_bam_host())
    assert "".join(bam) == text
    assert "".join(characterize.with_reference(bam, REF, host)) == calmd_lib.retagged(text, REF)


def check_tagged_text_errors(eng, tmp_path):
    recs = calmd_lib.random_records(seed=13, n=5, max_cols=100)
    text = calmd_lib.strip_tags(calmd_lib.sam_text(recs, REF))
    path = os.path.join(str(tmp_path), "e.sam")

    def fails(t, piece, ref=REF):
        with open(path, "w") as f:
            f.write(t)
        with pytest.raises(ValueError) as e:
            "".join(characterize.with_reference(path, ref, eng))
        assert piece in str(e.value) and path in str(e.value), str(e.value)
    fails(text.replace("LN:40000", "LN:40001"), "not the reference these reads were aligned to")
    fails(text.replace("\t%s\t" % REF.names[recs[0]["chrom"]], "\tchrZ\t", 1), "chrZ, which the reference does not hold")
    line = text.splitlines(True)[-1].split("\t")
    fails(text + "\t".join(line[:5] + ["3M2N3M"] + line[6:]), "a CIGAR op outside MIDSH=X")
    fails(text + "\t".join(["badpos"] + line[1:3] + ["0"] + line[4:]), "alignment badpos")
    other = model.make_reference(["chr_A.1", "chrB"], [REF.chrom(0)[:-1], REF.chrom(1)])
    fails(text, "@SQ SN:chr_A.1 has LN:110000, the reference has 109999", other)


def test_tagged_text_errors_on_the_host(host, tmp_path):
    check_tagged_text_errors(host, tmp_path)
    host.set_reference(REF)


# ---- training from input without tags ----------------------------------------------------------------------------------------------------
def training_files(eng, out_dir, source, hist: bool):
    """the files three stages write from `source` (a path or a SamSource): {name: bytes}"""
    os.makedirs(out_dir)
    prefix = os.path.join(out_dir, "training")
    if hist:
        characterize.hist(prefix, characterize.cs_from_sam(source), eng)
    characterize.base_qualities(prefix, *characterize.quals_from_sam(source), eng)
    characterize.homopolymer_lengths_from_sam(prefix, characterize.sam_records(source), eng)
    return {n: open(os.path.join(out_dir, n), "rb").read() for n in sorted(os.listdir(out_dir))}


def check_training_from_stripped_input(eng, tmp_path, hist: bool):
    """a SAM file with the generator's own tags against the same file without them through with_reference — as SAM text, as BAM, and
    with = / X ops in its CIGARs: the stages write the same files"""
    recs = calmd_lib.random_records(seed=21, n=120, max_cols=1500, hard=False)
    d = str(tmp_path)

    def written(name, text):
        path = os.path.join(d, name)
        with open(path, "w") as f:
            f.write(text)
        return path
    tagged = written("tagged.sam", calmd_lib.sam_text(recs, REF, unmapped=5))
    stripped = written("stripped.sam", calmd_lib.strip_tags(calmd_lib.sam_text(recs, REF, unmapped=5)))
    eqx_text = calmd_lib.sam_text(recs, REF, eqx=True, unmapped=5)
    eqx = written("eqx.sam", calmd_lib.strip_tags(eqx_text))
    eqx_md = written("eqx_md.sam", re.sub(r"\tcs:Z:[^\t\n]*", "", eqx_text))              # MD:Z stays: cs_of goes to get_cs
    bam = os.path.join(d, "stripped.bam")
    with open(bam, "wb") as f:
        f.write(bam_lib.sam_to_bam(open(stripped).read()))
    want = training_files(eng, os.path.join(d, "from_tagged"), tagged, hist)
    assert len(want) >= (11 if hist else 3) and all(want.values())
    for reader in (characterize.cs_from_sam, characterize.quals_from_sam):
        with pytest.raises(ValueError, match="neither a cs nor an MD tag"):
            reader(stripped)
    with pytest.raises(ValueError, match="has no MD tag"):
        characterize.sam_records(stripped)
    with pytest.raises(ValueError, match="not handled by get_cs"):
        characterize.cs_from_sam(eqx_md)
    sources = {"sam": characterize.with_reference(stripped, calmd_lib.GENOME, eng), "eqx": characterize.with_reference(eqx, calmd_lib.GENOME, eng),
               "bam": characterize.with_reference(characterize.read_bam(bam, eng), REF, eng)}
    for kind, source in sources.items():
        got = training_files(eng, os.path.join(d, "from_" + kind), source, hist)
        assert sorted(got) == sorted(want), kind
        for n in want:
            assert got[n] == want[n], (kind, n)


def test_training_from_stripped_input_on_the_host_builds(host, tmp_path):
    """base qualities and homopolymer lengths through the host builds of their walks (the characterisation histograms have no stand-in
    engine: the GPU test runs all three)"""
    from tests.test_bam import build_host as bam_host
    from tests.test_basequal import build_host_walk as qual_host
    from tests.test_sam_pairs import build_host_walk as pairs_host
    q, s, b = qual_host(), pairs_host(), bam_host()

    def check(rc):
        if rc:
            raise engine.EngineError("host walk: error %d" % rc)
    eng = types.SimpleNamespace(ctx=None, _check=check, set_reference=host.set_reference, L=types.SimpleNamespace(
        ns_calmd=host.L.ns_calmd, ns_qual_histograms=q.L.ns_qual_histograms, ns_sam_pairs_build=s.L.ns_sam_pairs_build,
        ns_hp_histograms_sam=s.L.ns_hp_histograms_sam, ns_hp_histograms=s.L.ns_hp_histograms, ns_bam_to_sam=b.L.ns_bam_to_sam))
    check_training_from_stripped_input(eng, tmp_path, hist=False)


# ---- the boundary -----------------------------------------------------------------------------------------------------------------------
def test_struct_layout_export_and_abi(host):
    out = os.path.join(ROOT, "tests", "_tmp")
    os.makedirs(out, exist_ok=True)
    c = os.path.join(out, "calmd_layout.c")
    with open(c, "w") as f:
        f.write('#include <stdio.h>\n#include <stddef.h>\n#include "nanosim_amd.h"\nint main(void) {\n'
                'printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(ns_calmd_result), offsetof(ns_calmd_result, md_off), offsetof(ns_calmd_result, cs),\n'
                '       offsetof(ns_calmd_result, cs_off), offsetof(ns_calmd_result, n_bad), offsetof(ns_calmd_result, first_bad),\n'
                '       offsetof(ns_calmd_result, bad_reason), offsetof(ns_calmd_result, ms_kernel));\n'
                'printf("%d %d %d %d %u\\n", NS_CALMD_BAD_CIGAR, NS_CALMD_BAD_SEQ_BYTE, NS_CALMD_BAD_END, NS_CALMD_BAD_NO_COLUMN, (unsigned)NS_ABI_VERSION);\nreturn 0; }\n')
    exe = os.path.join(out, "calmd_layout")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, c])
    a, b = subprocess.check_output([exe], text=True).strip().split("\n")
    R = characterize.NsCalmdResult
    assert [int(x) for x in a.split()] == [C.sizeof(R), R.md_off.offset, R.cs.offset, R.cs_off.offset, R.n_bad.offset, R.first_bad.offset, R.bad_reason.offset,
                                           R.ms_kernel.offset]
    assert [int(x) for x in b.split()] == [1, 5, 8, 9, model.NS_ABI_VERSION] and model.NS_ABI_VERSION == 7
    assert "ns_calmd" in engine.EXPORTS
    for name in ("with_reference", "calmd", "cs_md_call", "calmd_raw", "TaggedText", "NsCalmdResult", "CALMD_BAD_REASONS", "texts_of"):
        assert hasattr(characterize, name), name
    assert [host.constant(i) for i in range(4)] == [9, 1 << 28, 8, 16]
    src = open(os.path.join(ROOT, "nanosim_amd", "csrc", "ns_calmd.h")).read()
    assert "#define CALMD_MAX_DIGITS 9u" in src and "#define CALMD_SEQ_BYTES 8u" in src
