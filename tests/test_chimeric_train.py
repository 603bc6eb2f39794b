"""Training side, chimeric reads ("Chimeric reads: the split-alignment choice") on CPU: the engine's CIGAR readings and its
choice among split alignments (nanosim_amd/csrc/ns_chimeric.h, compiled for the host; on the GPU k_chim_scan and k_chim_select of
ns_train.h run them) and the host module around the calls — pinned against what the REAL src/get_primary_sam.py
(primary_and_unaligned_chimeric) collected and wrote for the same SAM text (tests/golden/reference_chimeric_train.json.gz,
tests/golden/make_chimeric_train_golden.py) and against hand-made reads with their expectations written out."""
import ctypes as C
import gzip
import json
import os
import subprocess
import types

import numpy as np
import pytest

from nanosim_amd import characterize, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO = characterize.CHIM_NO_GAP
POS, ALONE, HAS_SA = characterize.CHIM_POS_STRAND, characterize.CHIM_ALONE, characterize.CHIM_HAS_SA
BIG = 10 ** 9                                                # a reference on which nothing below is an edge
BAD_CIGARS = ("", "10", "M", "10Q", "10M5", "M10", "10MM", "4294967296M", "4294967295M1I", "2147483648M2147483648D", "*", "10M 5M")
GOOD_CIGARS = {"4294967295M": (0, 4294967295, 4294967295, 4294967295), "10M0I": (0, 10, 10, 10), "7S": (7, 7, 0, 0),
               "5S10M3I2D4N6X7=2P8S": (5, 18, 13, 12), "3H5S10M": (3, 13, 10, 10),
               "10=5S3M": (0, 3, 3, 3),                      # (`10=` leaves the item `1`,`0`: the first item is no clip)
               "5=3S4M": (3, 7, 4, 4),                       # (`5=` leaves no item: `3S` is the first)
               "12H100M4I50M9D3S": (12, 166, 154, 159)}


def load_fixture():
    with gzip.open(os.path.join(ROOT, "tests", "golden", "reference_chimeric_train.json.gz"), "rt") as f:
        fx = json.load(f)
    fx["refs"] = [tuple(r) for r in fx["refs"]]
    return fx


@pytest.fixture(scope="module")
def fx():
    return load_fixture()


def build_host_walk():
    """an object that stands in for an Engine: its ns_cigar_spans and ns_chimeric_select are the engine's walk compiled for the host
    (tests/chimeric_host.cpp)"""
    out = os.path.join(ROOT, "tests", "_tmp")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libchimeric_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tests", "chimeric_host.cpp")])
    L = C.CDLL(so)
    L.chim_host_cigar_spans.restype = C.c_int
    L.chim_host_cigar_spans.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.chim_host_chimeric_select.restype = C.c_int
    L.chim_host_chimeric_select.argtypes = [C.c_void_p] + [C.c_void_p] * 3 + [C.c_uint32] + [C.c_void_p] * 6 + [C.c_uint32, C.c_uint32, C.c_void_p]

    def check(rc):
        if rc:
            raise engine.EngineError("host walk: error %d" % rc)
    return types.SimpleNamespace(ctx=None, _check=check, L=types.SimpleNamespace(ns_cigar_spans=L.chim_host_cigar_spans,
                                                                                 ns_chimeric_select=L.chim_host_chimeric_select))


@pytest.fixture(scope="module")
def host():
    return build_host_walk()


def sam_file(fx, tmp_path):
    path = os.path.join(str(tmp_path), "training.sam")
    with open(path, "w") as f:
        f.write(fx["sam"])
    return path


SPECIES = {"spA_1": "spA", "spA_2": "spA", "spB_1": "spB"}


def check_fixture(eng, fx, tmp_path):
    """every quantity the reference recorded, in both species settings, exactly; -> the two results"""
    refs, records, unaligned_len, header = characterize.chimeric_records(sam_file(fx, tmp_path))
    assert refs == fx["refs"] and "".join(header) == fx["sam"][:len("".join(header))]
    got = {}
    for key, species in (("genome", None), ("meta", SPECIES)):
        exp = fx[key]
        g = got[key] = characterize.select_chimeric(eng, refs, records, species)
        assert unaligned_len.dtype == np.int64 and unaligned_len.tolist() == exp["unaligned_len"]
        assert g["gap_length"].dtype == np.int64 and g["gap_length"].tolist() == exp["gap_length"]
        assert [list(records[i][:5]) for i in g["selected"]] == [r[:5] for r in exp["written"]]
        assert [records[i].nm for i in g["selected"]] == exp["written_nm"]               # (which of two records with one key: the last)
        assert g["num_aligned"] == fx["n_reads"] and g["strandness"] == exp["strandness"] and g["pos_strand"] == round(exp["strandness"] * fx["n_reads"])
        assert g["n_pieces"].tolist() == fx["n_pieces"] and int(g["n_pieces"].sum()) == len(exp["written"])
        if species is None:
            assert g["species_count"] == {None: [len(exp["gap_length"]), 0]} and sum(c[0] for c in exp["species_count"].values()) == len(exp["gap_length"])
            beta = None
        else:
            assert g["species_count"] == exp["species_count"]
            beta = characterize.chimeric_beta(g["species_count"], fx["abundance"])
        assert characterize.format_chimeric_info(len(g["gap_length"]), g["num_aligned"], beta) == exp["chimeric_info"]
    return got


def test_host_walk_reproduces_the_reference(fx, host, tmp_path):
    assert fx["n_reads"] == 300 and len(fx["genome"]["gap_length"]) == 84 and len(fx["genome"]["written"]) == 402
    got = check_fixture(host, fx, tmp_path)
    g = got["genome"]
    names = list(dict.fromkeys(r[0] for r in fx["genome"]["written"]))
    flags = dict(zip(names, g["flags"].tolist()))
    pieces = dict(zip(names, g["n_pieces"].tolist()))
    t = fx["tags"]
    assert all(flags[n] & ALONE and pieces[n] == 1 for n in t["alone"]) and sum(1 for f in flags.values() if f & ALONE) == len(t["alone"])
    assert all(not flags[n] & HAS_SA for n in t["no_sa"]) and all(flags[n] & HAS_SA for n in t["alone"] + t["tie"] + t["positive_gap"])
    assert all(pieces[n] == 2 for n in t["circular_ES"] + t["circular_SE"] + t["no_primary_+"] + t["no_primary_-"] + t["lost_entry"])
    assert all(pieces[n] == 4 for n in t["four_pieces"]) and all(pieces[n] == 1 and not flags[n] & ALONE for n in t["same_qstart"] + t["tie"])
    assert all(flags[n] & POS for n in t["no_primary_+"]) and not any(flags[n] & POS for n in t["no_primary_-"])


def test_texts_against_the_fixture(fx):
    n, gaps = fx["n_reads"], len(fx["genome"]["gap_length"])
    assert characterize.format_chimeric_info(gaps, n) == fx["genome"]["chimeric_info"] == "Mean segments for each aligned read:\t1.28\n"
    beta = characterize.chimeric_beta(fx["meta"]["species_count"], fx["abundance"])
    assert characterize.format_chimeric_info(gaps, n, beta) == fx["meta"]["chimeric_info"] and not fx["meta"]["chimeric_info"].endswith("\n")
    assert characterize.chimeric_beta({"a": [3, 1], "b": [0, 0], "c": [1, 1]}, {"a": 50, "b": 25, "c": 25}) == (0.25 * 100 / 50 + 0.5 * 100 / 75) / 2
    with pytest.raises(ValueError):
        characterize.chimeric_beta({"a": [0, 0]}, {"a": 100})


# ---- hand-made reads ------------------------------------------------------------------------------------------------------------------------
def E(cigar, ref=0, start=5000, nm=0, rev=False):
    return (cigar, ref, start, nm, rev)


def call(eng, reads, ref_total=(BIG, BIG, BIG), species=(0, 0, 1), n_species=2):
    """chimeric_call as plain Python: per read (n_pieces, flags, [(entry, is_primary, gap)]), and the totals"""
    out, ent, pieces, per_read, count, ent_off = characterize.chimeric_call(eng, reads, ref_total, species, n_species)
    res = []
    for r in range(len(reads)):
        e0, k = int(ent_off[r]), int(per_read["n_pieces"][r])
        res.append((k, int(per_read["flags"][r]), [(int(p["entry"]), int(p["is_primary"]), int(p["gap"])) for p in pieces[e0:e0 + k]]))
    return types.SimpleNamespace(reads=res, n_gaps=int(out.n_gaps), pos_strand=int(out.pos_strand), n_bad=int(out.n_bad), first_bad=int(out.first_bad),
                                 count=count.tolist(), ent=ent, ent_off=ent_off)


# (name, the read, n_pieces, flags, pieces, n_gaps, pos_strand, species_count) — reference 2 is of the other species; LN = 10^9 unless said
HAND = [
    ("no SA, forward", [E("100M20S")], 1, POS, [(0, 1, NO)], 0, 1, [[0, 0], [0, 0]]),
    ("no SA, reverse", [E("100M20S", rev=True)], 1, 0, [(0, 1, NO)], 0, 0, [[0, 0], [0, 0]]),
    ("one compatible entry, a positive gap", [E("100M80S"), E("130S50M", 1)], 2, HAS_SA | POS, [(0, 1, NO), (1, 0, 30)], 1, 1, [[1, 0], [0, 0]]),
    ("... the primary second along the read", [E("130S50M", rev=True), E("100M80H", 2)], 2, HAS_SA, [(1, 0, NO), (0, 1, 30)], 1, 0, [[0, 0], [0, 1]]),
    ("a query overlap of 10: compatible, the gap clamped to 0", [E("100M80S"), E("90S50M", 1)], 2, HAS_SA | POS, [(0, 1, NO), (1, 0, 0)], 1, 1, [[1, 0], [0, 0]]),
    ("a query overlap of 11: a second list, which loses", [E("100M80S"), E("89S50M", 1)], 1, HAS_SA | POS, [(0, 1, NO)], 0, 1, [[0, 0], [0, 0]]),
    ("the second list wins alone: the primary is kept alone", [E("100M80S", nm=60), E("89S50M", 1)], 1, HAS_SA | ALONE | POS, [(0, 1, NO)], 0, 1, [[0, 0], [0, 0]]),
    ("... a reverse primary", [E("100M80S", nm=60, rev=True), E("89S50M", 1)], 1, HAS_SA | ALONE, [(0, 1, NO)], 0, 0, [[0, 0], [0, 0]]),
    ("a score tie: the first list", [E("100M80S", nm=50), E("89S50M", 1)], 1, HAS_SA | POS, [(0, 1, NO)], 0, 1, [[0, 0], [0, 0]]),
    ("scores are signed: -5 beats -6", [E("20M80S", nm=25), E("5S20M", 1, nm=26)], 1, HAS_SA | POS, [(0, 1, NO)], 0, 1, [[0, 0], [0, 0]]),
    ("a reference overlap on the same name: a second list", [E("100M80S", 0, 5000), E("130S50M", 0, 5040)], 1, HAS_SA | POS, [(0, 1, NO)], 0, 1, [[0, 0], [0, 0]]),
    ("... of 10 bases: compatible", [E("100M80S", 0, 5000), E("130S50M", 0, 5090)], 2, HAS_SA | POS, [(0, 1, NO), (1, 0, 30)], 1, 1, [[1, 0], [0, 0]]),
    ("... on another name: compatible", [E("100M80S", 0, 5000), E("130S50M", 2, 5040)], 2, HAS_SA | POS, [(0, 1, NO), (1, 0, 30)], 1, 1, [[0, 1], [0, 0]]),
    # B joins the primary's list and A's; A + B outscores primary + B: the winner holds no piece with the primary's qstart
    ("an entry in two lists; no primary, first-added +", [E("100M500S", nm=40, rev=True), E("50S200M", 1), E("300S100M", 2)], 2, HAS_SA | POS,
     [(1, 0, NO), (2, 0, 50)], 1, 1, [[0, 1], [0, 0]]),
    ("... first-added -: the direction list is not permuted", [E("100M500S", nm=40), E("50S200M", 1, rev=True), E("300S100M", 2)], 2, HAS_SA,
     [(1, 0, NO), (2, 0, 50)], 1, 0, [[0, 1], [0, 0]]),
    ("... first-added is later along the read", [E("100M500S", 0, 5000, nm=40), E("300S200M", 0, 5030, rev=True), E("150S100M", 2)], 2, HAS_SA,
     [(2, 0, NO), (1, 0, 50)], 1, 0, [[0, 0], [0, 1]]),
    ("an SA entry with the primary's qstart is the primary record", [E("100M500S", nm=40), E("300M", 1)], 1, HAS_SA | POS, [(1, 1, NO)], 0, 1, [[0, 0], [0, 0]]),
    ("H clips and = / X in an SA entry (neither counted)", [E("100M80S"), E("130H20=5X30M4I2D", 1, nm=3)], 2, HAS_SA | POS, [(0, 1, NO), (1, 0, 30)], 1, 1,
     [[1, 0], [0, 0]]),
    ("the primary's figures are pysam's: 5H10S, = and X", [E("5H10S50=40X80S"), E("110S50M", 1)], 2, HAS_SA | POS, [(0, 1, NO), (1, 0, 10)], 1, 1, [[1, 0], [0, 0]]),
    ("stable order among equal (qstart, qend)", [E("200S100M"), E("5S5M", 1), E("5S5M", 2), E("5S5M", 1, 9000)], 4, HAS_SA | POS,
     [(1, 0, NO), (2, 0, 0), (3, 0, 0), (0, 1, 190)], 3, 1, [[1, 1], [0, 1]]),
    ("two pieces with the primary's qstart count twice", [E("5S5M90S"), E("5S5M", 1)], 2, HAS_SA | POS, [(0, 1, NO), (1, 1, 0)], 1, 2, [[1, 0], [0, 0]]),
    # the SECOND inequality of G:38, `interval[1] - overlap_base > member[0]`, met with equality (the cases above meet the first with it):
    # the entry lies in FRONT of the member and ends 10 bases behind the member's start
    ("query axis: the entry ends 10 behind the primary's start: compatible", [E("100S100M50S"), E("50S60M", 1)], 2, HAS_SA | POS, [(1, 0, NO), (0, 1, 0)], 1, 1,
     [[1, 0], [0, 0]]),
    ("... 11 behind: a second list, which loses", [E("100S100M50S"), E("50S61M", 1)], 1, HAS_SA | POS, [(0, 1, NO)], 0, 1, [[0, 0], [0, 0]]),
    ("reference axis: the entry ends 10 behind the primary's start: compatible", [E("100M80S", 0, 5000), E("130S50M", 0, 4960)], 2, HAS_SA | POS,
     [(0, 1, NO), (1, 0, 30)], 1, 1, [[1, 0], [0, 0]]),
    ("... 11 behind: a second list, which loses", [E("100M80S", 0, 5000), E("130S50M", 0, 4961)], 1, HAS_SA | POS, [(0, 1, NO)], 0, 1, [[0, 0], [0, 0]]),
    # sorted() of G:338 compares (qstart, qend) tuples: among equal qstart the smaller qend comes first, whatever the entry order
    ("equal qstart, qend descending in entry order: sorted by qend", [E("200S100M"), E("5S8M", 1), E("5S5M", 2)], 3, HAS_SA | POS,
     [(2, 0, NO), (1, 0, 0), (0, 1, 187)], 2, 1, [[1, 0], [0, 1]]),
    ("... three of them, the middle one last", [E("200S100M"), E("5S9M", 1), E("5S3M", 2), E("5S6M", 1, 9000)], 4, HAS_SA | POS,
     [(2, 0, NO), (3, 0, 0), (1, 0, 0), (0, 1, 186)], 3, 1, [[2, 0], [0, 1]]),
]


@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_hand_made_reads(host, case):
    check_hand(host, case)


def check_hand(eng, case):
    _, read, k, flags, pieces, n_gaps, pos, count = case
    r = call(eng, [read])
    assert r.n_bad == 0 and r.reads == [(k, flags, pieces)] and (r.n_gaps, r.pos_strand, r.count) == (n_gaps, pos, count)


# the two ends of a circular reference of 5 000 bases (reference 0 here): rend >= 4599 is the end edge, start <= 400 the start edge
CIRCULAR = [
    ("end then start: skipped", [E("300M400S", 0, 4650), E("320S300M", 0, 100)], [(0, 1, NO), (1, 0, NO)], 0),
    ("start then end: skipped", [E("300M400S", 0, 100), E("320S300M", 0, 4650)], [(0, 1, NO), (1, 0, NO)], 0),
    ("another name: recorded", [E("300M400S", 0, 4650), E("320S300M", 1, 100)], [(0, 1, NO), (1, 0, 20)], 1),
    ("start and start: recorded", [E("300M400S", 0, 100), E("320S300M", 0, 3000)], [(0, 1, NO), (1, 0, 20)], 1),
    ("a piece of 99 reference bases is no edge: recorded", [E("300M400S", 0, 4650), E("320S99M", 0, 100)], [(0, 1, NO), (1, 0, 20)], 1),
    ("100 reference bases are", [E("300M400S", 0, 4650), E("320S100M", 0, 100)], [(0, 1, NO), (1, 0, NO)], 0),
    ("the end edge wins over the start edge (elif)", [E("300M400S", 0, 4720), E("320S4400M", 0, 300)], [(0, 1, NO), (1, 0, 20)], 1),
    ("the primary's own length is M + D + N + = + X", [E("50M30N20=400S", 0, 4650), E("320S300M", 0, 100)], [(0, 1, NO), (1, 0, NO)], 0),
    ("the edge of the PREVIOUS piece counts, not the first's", [E("300M900S", 0, 4650), E("320S300M", 1, 100), E("640S300M", 0, 100)],
     [(0, 1, NO), (1, 0, 20), (2, 0, 20)], 2),
]


@pytest.mark.parametrize("case", CIRCULAR, ids=[c[0] for c in CIRCULAR])
def test_circular_joins(host, case):
    check_circular(host, case)


def check_circular(eng, case):
    _, read, pieces, n_gaps = case
    r = call(eng, [read], ref_total=(5000, 5000, BIG))
    assert r.reads[0][2] == pieces and r.n_gaps == n_gaps and sum(map(sum, r.count)) == n_gaps


def many_compatible(n):
    """a read whose n SA entries are all compatible, listed from the last along the read to the first: one list, n + 1 pieces, and what
    the call has to give for it"""
    read = [E("100M%dS" % (105 * n), 0, 1000)] + [E("%dS100M" % (105 * i), i % 3, 1000 + 500 * i, nm=i % 7) for i in range(n, 0, -1)]
    pieces = [(0, 1, NO)] + [(n + 1 - i, 0, 5) for i in range(1, n + 1)]
    return read, pieces


def many_overlapping(n, winner):
    """a read whose n SA entries all overlap each other and the primary: n + 1 lists of one; entry `winner` has the best score"""
    return [E("1000M", 0, 1000, nm=500)] + [E("1S%dM" % (900 + e), e % 3, 7000 * e, nm=0 if e == winner else 800) for e in range(1, n + 1)]


@pytest.mark.parametrize("n", [63, 64, 65, 130])
def test_reads_at_the_mask_word_borders(host, n):
    check_mask_borders(host, n)


def check_mask_borders(eng, n):
    read, pieces = many_compatible(n)
    lone = [E("100M")]
    r = call(eng, [lone, read, lone, many_overlapping(n, n), many_overlapping(n, 64 if n >= 64 else 1), many_overlapping(n, 0), lone])
    assert r.n_bad == 0 and r.reads[1] == (n + 1, HAS_SA | POS, pieces)
    assert r.reads[3] == r.reads[4] == (1, HAS_SA | ALONE | POS, [(0, 1, NO)])               # (a list of one that is not the primary)
    assert r.reads[5] == (1, HAS_SA | POS, [(0, 1, NO)])                                     # (every entry scores below the primary: list 0)
    assert r.reads[0] == r.reads[2] == r.reads[6] == (1, POS, [(0, 1, NO)])
    assert (r.n_gaps, r.pos_strand) == (n, 7)
    by_species = [[0, 0], [0, 0]]
    order = [0] + [n + 1 - i for i in range(1, n + 1)]
    sp = lambda e: (0, 0, 1)[read[e][1]]
    for a, b in zip(order, order[1:]):
        by_species[sp(a)][0 if sp(a) == sp(b) else 1] += 1
    assert r.count == by_species


def test_cigar_readings(host):
    cigars = list(GOOD_CIGARS)
    got, n_bad, first_bad, _ = characterize.cigar_spans(host, cigars)
    assert n_bad == 0 and first_bad == len(cigars)
    assert [tuple(int(v) for v in g) for g in got] == [GOOD_CIGARS[c] for c in cigars]
    # pysam's reading, through the primary of a read
    r = call(host, [[E("5S10M3I2D4N6X7=2P8S")], [E("3H5S10M")], [E("10=5S3M")], [E("5S2H3S10M")]])
    assert [tuple(int(v) for v in r.ent[int(i)]) for i in r.ent_off[:-1]] == [(5, 31, 26, 29), (5, 15, 10, 10), (0, 13, 13, 13), (8, 18, 10, 10)]
    assert characterize.cigar_spans(host, [])[1:3] == (0, 0)


@pytest.mark.parametrize("bad", BAD_CIGARS, ids=[repr(b) for b in BAD_CIGARS])
def test_bad_cigars(host, bad):
    check_bad(host, bad)


def check_bad(eng, bad):
    got, n_bad, first_bad, _ = characterize.cigar_spans(eng, ["10M", bad, "5S3M", bad])
    assert (n_bad, first_bad) == (2, 1) and [tuple(int(v) for v in g) for g in got] == [(0, 10, 10, 10), (0, 0, 0, 0), (5, 8, 3, 3), (0, 0, 0, 0)]
    for where in (0, 1, 2):                                   # the primary, the middle entry, the last entry of the middle read
        reads = [[E("50M")], [E("100M80S"), E("130S50M", 1), E("20S30M", 2)], [E("60M")]]
        reads[1][where] = E(bad, reads[1][where][1])
        r = call(eng, reads)
        assert (r.n_bad, r.first_bad) == (1, 1 + where) and not r.ent[1 + where].tolist()[0] and not any(r.ent[1 + where].tolist())


def check_cigar_bleed(eng):
    """a count without an op directly in front of a CIGAR that begins with an op letter (the CIGARs of a call lie one behind the other):
    both are bad, each on its own, in both readings"""
    cigars = ["7M", "10", "M", "3S4M", "12M5", "S5M", "6", "I2M", "9M"]
    want = [(0, 7, 7, 7), (0, 0, 0, 0), (0, 0, 0, 0), (3, 7, 4, 4), (0, 0, 0, 0), (0, 0, 0, 0), (0, 0, 0, 0), (0, 0, 0, 0), (0, 9, 9, 9)]
    got, n_bad, first_bad, _ = characterize.cigar_spans(eng, cigars)
    assert (n_bad, first_bad) == (6, 1) and [tuple(int(v) for v in g) for g in got] == want
    r = call(eng, [[E("10")], [E("M")], [E("50M")], [E("100M80S"), E("130S5", 1), E("M50M", 2)]])          # ... and as a read's entries
    assert (r.n_bad, r.first_bad) == (4, 0) and [tuple(int(v) for v in e) for e in r.ent] == [(0, 0, 0, 0)] * 2 + [(0, 50, 50, 50), (0, 100, 100, 100)] + [(0, 0, 0, 0)] * 2


def test_a_cigar_that_ends_early_does_not_borrow_from_its_neighbour(host):
    check_cigar_bleed(host)


# ---- the host module ---------------------------------------------------------------------------------------------------------------------------
HEAD = "@HD\tVN:1.6\n@SQ\tSN:chrA\tLN:50000\n@SQ\tSN:chrB\tLN:5000\n"


def line(q, flag, rname, pos, cigar, *tags, seq="*"):
    return "\t".join([q, str(flag), rname, str(pos), "60", cigar, "*", "0", "0", seq, "*"] + list(tags)) + "\n"


def write(tmp_path, text):
    path = os.path.join(str(tmp_path), "in.sam")
    with open(path, "w") as f:
        f.write(text)
    return path


def test_chimeric_records_and_its_errors(tmp_path):
    ok = HEAD + line("u0", 4, "*", 0, "*", seq="ACGTA") + line("r1", 0, "chrA", 100, "100M80S", "NM:i:3", "SA:Z:chrB,200,-,130S50M,60,2;") + \
        line("r1", 2064, "chrB", 200, "130S50M", "NM:i:2") + line("u1", 4, "*", 0, "*") + line("r2", 16, "chrB", 7, "50M", "AS:i:9", "NM:i:0")
    refs, recs, unaligned, header = characterize.chimeric_records(write(tmp_path, ok))
    assert refs == [("chrA", 50000), ("chrB", 5000)] and "".join(header) == HEAD and unaligned.tolist() == [5, 0]
    assert [tuple(r[:8]) for r in recs] == [("r1", 0, "chrA", 100, "100M80S", 3, "chrB,200,-,130S50M,60,2;", 0), ("r1", 2064, "chrB", 200, "130S50M", 2, None, 0),
                                           ("r2", 16, "chrB", 7, "50M", 0, None, 0)]
    assert "".join(r.line for r in recs) == "".join(l + "\n" for l in ok[len(HEAD):].split("\n") if l and "\t4\t" not in l)
    assert characterize.sa_entries("chrB,200,-,130S50M,60,2;chrA,7,+,5M,0,1") == [("chrB", 199, True, "130S50M", 2)]        # (no closing `;`: the last is lost)
    for what, text in (("no NM", HEAD + line("r1", 0, "chrA", 100, "100M")),
                       ("six", HEAD + line("r1", 0, "chrA", 100, "100M", "NM:i:1", "SA:Z:chrB,200,-,130S50M,60;")),
                       ("six", HEAD + line("r1", 0, "chrA", 100, "100M", "NM:i:1", "SA:Z:chrB,200,-,130S50M,60,2,9;")),
                       ("@SQ", HEAD + line("r1", 0, "chrC", 100, "100M", "NM:i:1")),
                       ("@SQ", HEAD + line("r1", 0, "chrA", 100, "100M", "NM:i:1", "SA:Z:chrC,200,-,130S50M,60,2;")),
                       ("in front of the first primary", HEAD + line("r1", 2048, "chrA", 100, "100M", "NM:i:1") + line("r1", 0, "chrA", 100, "100M", "NM:i:1")),
                       ("in front of the first primary", HEAD + line("r1", 256, "chrA", 100, "100M") + line("r1", 0, "chrA", 100, "100M", "NM:i:1")),
                       ("no primary", HEAD + line("u0", 4, "*", 0, "*", seq="ACGT")),
                       ("no primary", HEAD)):
        with pytest.raises(ValueError, match=what):
            characterize.chimeric_records(write(tmp_path, text))


def test_select_matches_records_as_the_reference_does(host, tmp_path):
    sa = "SA:Z:chrB,200,-,130S50M,60,2;"
    prim = line("r1", 0, "chrA", 100, "100M80S", "NM:i:3", sa)
    nxt = line("r2", 0, "chrA", 900, "100M", "NM:i:0")
    match = lambda q, flag, nm: line(q, flag, "chrB", 200, "130S50M", "NM:i:%d" % nm)

    def selected(text):
        refs, recs, _, _ = characterize.chimeric_records(write(tmp_path, HEAD + text))
        s = characterize.select_chimeric(host, refs, recs)
        return [(recs[i].qname, recs[i].flag, recs[i].nm) for i in s["selected"]], s
    got, s = selected(prim + match("r1", 2064, 2) + nxt)
    assert got == [("r1", 0, 3), ("r1", 2064, 2), ("r2", 0, 0)] and s["gap_length"].tolist() == [30] and s["strandness"] == 1.0 and s["n_pieces"].tolist() == [2, 1]
    assert selected(prim + match("r1", 272, 2) + nxt)[0][1] == ("r1", 272, 2)                                    # a secondary record matches
    assert selected(prim + match("r1", 2064, 2) + match("r1", 272, 7) + nxt)[0][1] == ("r1", 272, 7)             # two match: the last
    assert selected(prim + match("other", 2064, 5) + nxt)[0][1] == ("other", 2064, 5)                            # whatever its QNAME
    assert selected(prim + line("r1", 2064, "chrB", 200, "130H40M5I5M3D", "NM:i:4") + nxt)[0][1] == ("r1", 2064, 4)   # equal figures are enough
    for text in (prim + nxt + match("r1", 2064, 2),                                                               # behind the next primary
                 prim + line("r1", 2064, "chrB", 201, "130S50M", "NM:i:2") + nxt, prim + line("r1", 2064, "chrA", 200, "130S50M", "NM:i:2") + nxt,
                 prim + line("r1", 2064, "chrB", 200, "130S51M", "NM:i:2") + nxt, prim + nxt):
        with pytest.raises(ValueError, match="read r1"):
            selected(text)
    with pytest.raises(ValueError, match="CIGAR"):
        selected(line("r1", 0, "chrA", 100, "100M80S", "NM:i:3", "SA:Z:chrB,200,-,130S5Q,60,2;") + nxt)
    with pytest.raises(ValueError, match="CIGAR"):
        selected(prim + match("r1", 2064, 2) + line("r1", 256, "chrB", 200, "*", "NM:i:2") + nxt)
    # a species mapping: the gap lies behind a chrA piece and in front of a chrB piece
    refs, recs, _, _ = characterize.chimeric_records(write(tmp_path, HEAD + prim + match("r1", 2064, 2) + nxt))
    assert characterize.select_chimeric(host, refs, recs, {"chrA": "a", "chrB": "b"})["species_count"] == {"a": [0, 1], "b": [0, 0]}
    assert characterize.select_chimeric(host, refs, recs, {"chrA": "a", "chrB": "a"})["species_count"] == {"a": [1, 0]}
    assert characterize.species_of_reference("Escherichia_coli_chr1") == "Escherichia_coli" and characterize.species_of_reference("chr1") == ""


def test_chimeric_writes_its_files_and_merges_the_npz(fx, host, tmp_path):
    prefix = os.path.join(str(tmp_path), "training")
    np.savez(prefix + "_kde.npz", aligned_reads_data=np.array([1.0, 2.0]), aligned_reads_bw=np.float64(10), gap_length_data=np.array([9.0]), gap_length_bw=np.float64(3))
    refs, recs, unaligned_len, strandness = characterize.chimeric(prefix, sam_file(fx, tmp_path), host, pickles=False)
    with open(prefix + "_chimeric_info") as f:
        assert f.read() == fx["genome"]["chimeric_info"]
    with np.load(prefix + "_kde.npz") as z:
        assert sorted(z.files) == ["aligned_reads_bw", "aligned_reads_data", "gap_length_bw", "gap_length_data"]
        assert z["aligned_reads_data"].tolist() == [1.0, 2.0] and float(z["aligned_reads_bw"]) == 10.0 and float(z["gap_length_bw"]) == 0.01
        assert np.array_equal(z["gap_length_data"], np.log10(np.array(fx["genome"]["gap_length"], dtype=np.int64) + 1))
    assert refs == fx["refs"] and [list(r) for r in recs] == [r[:5] for r in fx["genome"]["written"]] and strandness == fx["genome"]["strandness"]
    assert unaligned_len.tolist() == fx["genome"]["unaligned_len"]
    # <prefix>_primary.sam: what the existing readers see is what the reference's later steps see in <prefix>_primary.bam
    refs2, recs2 = characterize.length_records(prefix + "_primary.sam")
    assert refs2 == refs and recs2 == recs
    lines = set(l for l in fx["sam"].splitlines(True) if not l.startswith("@"))
    with open(prefix + "_primary.sam") as f:
        body = [l for l in f if not l.startswith("@")]
    assert all(l in lines for l in body) and len(body) == len(recs)
    # write_kde as before: without merge the file holds the models alone; with it the other keys stay
    characterize.write_kde(prefix, {"ht_ratio": (np.array([0.5]), 0.01)}, pickles=False, merge=True)
    with np.load(prefix + "_kde.npz") as z:
        assert len(z.files) == 6
    characterize.write_kde(prefix, {"ht_ratio": (np.array([0.5]), 0.01)}, pickles=False)
    with np.load(prefix + "_kde.npz") as z:
        assert sorted(z.files) == ["ht_ratio_bw", "ht_ratio_data"]
    with pytest.raises(ValueError):
        characterize.chimeric(prefix, sam_file(fx, tmp_path), host, abundance={"spA": 50, "spB": 50})
    characterize.chimeric(prefix, sam_file(fx, tmp_path), host, species=SPECIES, abundance=fx["abundance"], primary_sam=False, pickles=False)
    with open(prefix + "_chimeric_info") as f:
        assert f.read() == fx["meta"]["chimeric_info"]


def test_struct_layouts_and_exports(tmp_path):
    src = os.path.join(str(tmp_path), "layout.c")
    with open(src, "w") as f:
        f.write('''#include <stdio.h>
#include <stddef.h>
#include "nanosim_amd.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(ns_chim_result), offsetof(ns_chim_result, ent), offsetof(ns_chim_result, pieces),
         offsetof(ns_chim_result, reads), offsetof(ns_chim_result, species_count), offsetof(ns_chim_result, n_gaps), offsetof(ns_chim_result, pos_strand),
         offsetof(ns_chim_result, n_bad), offsetof(ns_chim_result, first_bad), offsetof(ns_chim_result, ms_kernel), offsetof(ns_chim_result, ms_scan));
  printf("%zu %zu %zu %zu %zu\\n", sizeof(ns_chim_ent), offsetof(ns_chim_ent, qstart), offsetof(ns_chim_ent, qend), offsetof(ns_chim_ent, qlen), offsetof(ns_chim_ent, rlen));
  printf("%zu %zu %zu %zu\\n", sizeof(ns_chim_piece), offsetof(ns_chim_piece, entry), offsetof(ns_chim_piece, is_primary), offsetof(ns_chim_piece, gap));
  printf("%zu %zu %zu %d %u %u %u\\n", sizeof(ns_chim_read), offsetof(ns_chim_read, n_pieces), offsetof(ns_chim_read, flags), NS_CHIM_NO_GAP,
         NS_CHIM_POS_STRAND, NS_CHIM_ALONE, NS_CHIM_HAS_SA);
  return 0;
}
''')
    exe = os.path.join(str(tmp_path), "layout")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
    rows = [[int(v) for v in l.split()] for l in subprocess.check_output([exe]).decode().splitlines()]
    R = characterize.NsChimResult
    assert rows[0] == [C.sizeof(R)] + [getattr(R, n).offset for n, _ in R._fields_]
    for row, dt in zip(rows[1:4], (characterize.CHIM_ENT_DTYPE, characterize.CHIM_PIECE_DTYPE, characterize.CHIM_READ_DTYPE)):
        assert row[:1 + len(dt.names)] == [dt.itemsize] + [dt.fields[n][1] for n in dt.names]
    assert rows[3][3:] == [NO, POS, ALONE, HAS_SA]
    assert "ns_cigar_spans" in engine.EXPORTS and "ns_chimeric_select" in engine.EXPORTS
    with open(os.path.join(ROOT, "include", "nanosim_amd.h")) as f:
        assert "#define NS_ABI_VERSION 7u" in f.read()        # added functions, no ABI bump


def test_host_walk_is_clean_under_the_sanitizers(fx, tmp_path):
    """the walk as a stand-alone program with -fsanitize=address,undefined, on the fixture's entries (exact-size buffers: a byte read
    past a CIGAR or a word past the workspace is an error) and on the mask-border reads"""
    refs, records, _, _ = characterize.chimeric_records(sam_file(fx, tmp_path))
    index = {n: i for i, (n, _) in enumerate(refs)}
    rows = ["%d" % len(refs)] + ["%d %d" % (ln, 0 if n.startswith("spA") else 1) for n, ln in refs]
    n_reads = 0
    for r in records:
        if r.flag & (0x100 | 0x800):
            continue
        n_reads += 1
        rows.append("1 %d %d %d %d %s" % (1 if r.flag & 16 else 0, index[r.rname], r.pos - 1, r.nm, r.cigar))
        for e in characterize.sa_entries(r.sa, r.qname) if r.sa else []:
            rows.append("0 %d %d %d %d %s" % (1 if e[2] else 0, index[e[0]], e[1], e[4], e[3]))
    for n in (63, 64, 65, 130):
        for read in (many_compatible(n)[0], many_overlapping(n, n)):
            rows += ["%d %d %d %d %d %s" % (1 if i == 0 else 0, 1 if e[4] else 0, e[1], e[2], e[3], e[0]) for i, e in enumerate(read)]
    rows.append("1 0 0 5 0 -")                                # an empty CIGAR: bad
    path = os.path.join(str(tmp_path), "entries.txt")
    with open(path, "w") as f:
        f.write("\n".join(rows) + "\n")
    exe = os.path.join(str(tmp_path), "chimeric_host_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DCHIMERIC_MAIN", "-o", exe,
                           os.path.join(ROOT, "tests", "chimeric_host.cpp")])
    out = subprocess.run([exe, path], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    first = [int(v) for v in out.stdout.splitlines()[0].split()]
    n_ent = len(rows) - 1 - len(refs)
    assert first[0] == len(fx["meta"]["gap_length"]) + 63 + 64 + 65 + 130 and first[2:] == [1, n_ent - 1]
