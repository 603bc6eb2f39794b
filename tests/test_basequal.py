"""Training side, the base-quality model on CPU: the engine's walk over cs + QUAL (nanosim_amd/csrc/ns_qual_hist.h, compiled
for the host; on the GPU the kernels of ns_train.h run it), the closed-form log-normal fit and the host module around the call — pinned against what the REAL
src/model_base_qualities.py collected and wrote for the same alignments (tests/golden/reference_basequal.json.gz,
tests/golden/make_basequal_golden.py) and against a per-base expansion written here."""
import ctypes as C
import gzip
import json
import os
import re
import shutil
import subprocess
import tempfile
import types

import numpy as np
import pytest

from nanosim_amd import characterize, engine, model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPES = ("mis", "ins", "match", "ht", "unmapped")
REL_TOL = 1e-12        # sd and mu: both sides evaluate the same closed form; summation order only (pairwise over <= 5e5 terms against 94: ~1e-14)


def load_fixture():
    with gzip.open(os.path.join(ROOT, "tests", "golden", "reference_basequal.json.gz"), "rt") as f:
        fx = json.load(f)
    fx["alignments"] = [tuple(a) for a in fx["alignments"]]
    fx["hist"] = np.array([fx["hist"][t] for t in TYPES], dtype=np.uint64)
    return fx


@pytest.fixture(scope="module")
def fx():
    return load_fixture()


def build_host_walk():
    """an object that stands in for an Engine: its ns_qual_histograms is the engine's walk compiled for the host (tests/qual_hist_host.cpp)"""
    out = os.path.join(ROOT, "tests", "_tmp")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libqual_hist_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tests", "qual_hist_host.cpp")])
    L = C.CDLL(so)
    L.qh_host_histograms.restype = C.c_int
    L.qh_host_histograms.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]

    def check(rc):
        if rc:
            raise engine.EngineError("host walk: error %d" % rc)
    return types.SimpleNamespace(ctx=None, L=types.SimpleNamespace(ns_qual_histograms=L.qh_host_histograms), _check=check)


@pytest.fixture(scope="module")
def host():
    return build_host_walk()


def raw_counts(eng, entries):
    """(hist (5, 94), n_short, n_bad_qual, the columns behind 93 all zero) of [(cs, qual, head, tail, unmapped)] in this order"""
    h = characterize._qual_call(eng, entries)
    full = np.ctypeslib.as_array(h.hist).copy()
    assert not full[:, 94:].any()
    return full[:, :94], int(h.n_short), int(h.n_bad_qual)


def brute_force(entries):
    """the reference's way, restated: the cs string expanded into one entry per query base (convert_cs), then base by base"""
    hist = np.zeros((5, 94), dtype=np.uint64)
    n_short = 0
    for cs, qual, head, tail, unmapped in entries:
        q = [ord(c) - 33 for c in qual]
        if unmapped:
            for v in q:
                hist[4][v] += 1
            continue
        arr = []
        for item in re.findall(r'(:[0-9]+|\*[a-z][a-z]|[=\+\-][A-Za-z]+)', cs):
            if item[0] == ":":
                arr += [2] * int(item[1:])
            elif item[0] == "+":
                arr += [1] * (len(item) - 1)
            elif item[0] == "*":
                arr += [0]
        aligned = q[head:len(q) - tail]
        if len(arr) < len(aligned):
            n_short += 1
            arr += [2] * len(aligned)
        for i, v in enumerate(aligned):
            hist[arr[i]][v] += 1
        for v in q[:head] + q[len(q) - tail:]:
            hist[3][v] += 1
    return hist, n_short


CORNERS = [(":57", 57), ("*ag", 1), ("+acgt", 4), ("*ag:5*ct", 7), ("+a:5+c", 7), (":3+acgtacgtacgtacgtacgtacg:4", 30), (":10+ACGT:5~gt12ag:6", 25),
           ("x:4??*ag;:3", 8), (":50*ag:50", 30), (":5+acgtacgt:5", 8), (":6-acg:6-t*ag:2", 15), (":4=ACG:2", 6), (":12", 0), ("", 0),
           ("::7*a1*ab:3", 11), (":0:0*ag:0", 1), (":100000", 100),
           # items left over exactly when the cursor stands AT the aligned length (a mismatch or an insertion taken there would mark the
           # first base of the next alignment: each of these is followed by one that begins with a match), and strings that end exactly there
           (":4*ag:2", 4), (":3*ag+acg", 4), (":2+ac*ag:1", 4), (":4*ag", 5), (":1*ag*ct+a", 2), (":5+ac", 7), (":3+acg+t*ag", 6), (":7", 7)]


def random_entries(rng, n):
    """random cs strings (every item kind, junk) with a QUAL of the length they cover (sometimes cut), clips, unmapped entries in between"""
    out = []
    for _ in range(n):
        if rng.random() < 0.15:
            out.append(("", "".join(chr(33 + int(v)) for v in rng.integers(0, 94, int(rng.integers(0, 70)))), 0, 0, 1))
            continue
        items, cover = [], 0
        for _ in range(int(rng.integers(0, 12))):
            k = rng.integers(0, 6)
            if k == 0:
                m = int(rng.integers(0, 40)); items.append(":%d" % m); cover += m
            elif k == 1:
                items.append("*" + "".join(rng.choice(list("acgt"), 2))); cover += 1
            elif k == 2:
                m = int(rng.integers(1, 25)); items.append("+" + "".join(rng.choice(list("acgtACGT"), m))); cover += m
            elif k == 3:
                items.append("-" + "".join(rng.choice(list("acgt"), int(rng.integers(1, 6)))))
            elif k == 4:
                items.append("=" + "".join(rng.choice(list("ACGT"), int(rng.integers(1, 6)))))
            else:
                items.append("".join(rng.choice(list("~;?*:+-1a"), int(rng.integers(1, 3)))))
        cs = "".join(items)
        cover = len(brute_cover(cs))
        aligned = cover if rng.random() < 0.7 else int(rng.integers(0, cover + 1))
        head, tail = (int(rng.integers(0, 20)), int(rng.integers(0, 20))) if rng.random() < 0.7 else (0, 0)
        out.append((cs, "".join(chr(33 + int(v)) for v in rng.integers(0, 94, head + aligned + tail)), head, tail, 0))
    return out


def brute_cover(cs):
    return [1 for item in re.findall(r'(:[0-9]+|\*[a-z][a-z]|[=\+\-][A-Za-z]+)', cs)
            for _ in range(int(item[1:]) if item[0] == ":" else len(item) - 1 if item[0] == "+" else 1 if item[0] == "*" else 0)]


def offset_entries(rng):
    """one call whose cs strings begin at every offset 0 .. 7 mod 8 of the packed bytes with every length 0 .. 17
    (tests/test_characterize.py: every_offset_and_length), each with a QUAL of the length it covers: so do the quality strings, nearly"""
    from tests.test_characterize import CS_FILLER, CS_PATTERN, every_offset_and_length
    cs, where = every_offset_and_length(CS_PATTERN, CS_FILLER)
    off = np.cumsum([0] + [len(c) for c in cs])
    assert {(int(off[i]) % 8, len(cs[i])) for i in where} == {(o, n) for o in range(8) for n in range(18)}
    return [(c, "".join(chr(33 + int(v)) for v in rng.integers(0, 94, len(brute_cover(c)))), 0, 0, 0) for c in cs]


def check_offset_entries(eng):
    rng = np.random.default_rng(17)
    entries = offset_entries(rng)
    for e in (entries, entries[::-1]):
        hist, n_short, n_bad = raw_counts(eng, e)
        exp, exp_short = brute_force(e)
        assert n_bad == 0 and n_short == exp_short == 0 and np.array_equal(hist, exp)
        assert hist[0].sum() > 100 and hist[1].sum() > 100


def test_cs_strings_at_every_offset_and_length(host):
    check_offset_entries(host)


def fixture_entries(fx):
    return [(c, q, h, t, 0) for c, q, h, t in fx["alignments"]] + [("", q, 0, 0, 1) for q in fx["unmapped"]]


def same_file(text, ref_text):
    """the reference's file: header, names and the loc column as text; sd and mu within REL_TOL"""
    got, ref = text.split("\n"), ref_text.split("\n")
    assert len(got) == len(ref) == 7 and got[0] == ref[0] == "type\tsd\tloc\tmu" and got[6] == ref[6] == ""
    for g, r in zip(got[1:6], ref[1:6]):
        g, r = g.split("\t"), r.split("\t")
        assert len(g) == len(r) == 4 and g[0] == r[0] and g[2] == r[2] == "0"
        for i in (1, 3):
            assert abs(float(g[i]) - float(r[i])) <= REL_TOL * abs(float(r[i])), (g, r)
    assert [line.split("\t")[0] for line in got[1:6]] == list(TYPES) == list(characterize.QUAL_TYPES)


def test_host_walk_equals_what_the_reference_collected(fx, host):
    hist, n_short, n_bad = raw_counts(host, fixture_entries(fx))
    assert n_short == 0 and n_bad == 0
    assert np.array_equal(hist, fx["hist"])
    t = characterize.count_qualities(host, fx["alignments"], fx["unmapped"])
    assert t["hist"].dtype == np.uint64 and t["hist"].shape == (5, 94) and np.array_equal(t["hist"], fx["hist"])


def test_host_walk_equals_the_per_base_expansion(fx, host):
    rng = np.random.default_rng(11)
    corners = [(cs, "".join(chr(33 + int(v)) for v in rng.integers(1, 94, 3 + n + 2)), 3, 2, 0) for cs, n in CORNERS]
    corners += [(cs, "".join(chr(33 + int(v)) for v in rng.integers(1, 94, n)), 0, 0, 0) for cs, n in CORNERS]
    for entries in (corners, [e for e in corners if e[1]][::-1], random_entries(rng, 400), fixture_entries(fx)[:10]):
        hist, n_short, n_bad = raw_counts(host, entries)
        exp, exp_short = brute_force(entries)
        assert n_bad == 0 and n_short == exp_short
        assert np.array_equal(hist, exp)
    for e in corners:                                            # ... and one by one (a wrong count can cancel in a sum)
        assert np.array_equal(raw_counts(host, [e])[0], brute_force([e])[0]), e


def test_fit_and_format_equal_the_reference_file(fx):
    same_file(characterize.format_base_qualities(characterize.fit_qualities(fx["hist"])), fx["file"])
    # a class mix-up would show: the five rows differ by far more than the tolerance
    p = characterize.fit_qualities(fx["hist"])
    assert len({round(p[t][2], 1) for t in TYPES}) == 5


def test_value_errors(fx, host):
    h = fx["hist"].copy()
    h[1] = 0
    with pytest.raises(ValueError, match="'ins'"):
        characterize.fit_qualities(h)
    h = fx["hist"].copy()
    h[3][0] = 1
    with pytest.raises(ValueError, match="'ht'"):
        characterize.fit_qualities(h)
    with pytest.raises(ValueError, match="fewer query bases"):                       # cs covers 9 of 10 aligned bases
        characterize.count_qualities(host, [(":4*ag:4", "I" * 13, 2, 1)])
    assert raw_counts(host, [(":4*ag:4", "I" * 13, 2, 1, 0), (":3", "III", 0, 0, 0), ("", "I" * 9, 0, 0, 1)])[1] == 1
    with pytest.raises(ValueError, match="outside"):
        characterize.count_qualities(host, [(":3", "I I", 0, 0)])
    hist, n_short, n_bad = raw_counts(host, [(":3", "I\x7fI", 0, 0, 0), ("", " !~", 0, 0, 1)])
    assert n_bad == 2 and hist.sum() == 4 and hist[4][0] == 1 and hist[4][93] == 1
    assert characterize.count_qualities(host, [])["hist"].sum() == 0


def test_quals_from_sam(tmp_path):
    sam = tmp_path / "a.sam"
    rec = lambda name, flag, cigar, qual, *tags: "\t".join([name, str(flag), "chr", "1", "60", cigar, "*", "0", "0", "A" * (len(qual) if qual != "*" else 4), qual] + list(tags)) + "\n"
    sam.write_text("@HD\tVN:1.6\n@SQ\tSN:chr\tLN:1000\n" +
                   rec("fwd", 0, "2S10M3S", "ABCDEFGHIJKLMNO", "cs:Z::4*ag:5") +
                   rec("rev", 16, "5M2I5M", "abcdefghijkl", "NM:i:2", "MD:Z:10") +                       # cs from CIGAR + MD
                   rec("unm", 4, "*", "!!~~") +
                   rec("unm_noqual", 4, "*", "*") +                                                     # skipped (P:174)
                   rec("sec", 256, "10M", "KKKKKKKKKK", "cs:Z::10") +
                   rec("sup", 2048, "4H6M2S", "LLLLLLLL", "cs:Z::6") +
                   rec("hard", 0, "3H1S6M2H", "MNOPQRS", "cs:Z::6"))
    aligned, unmapped = characterize.quals_from_sam(str(sam))
    assert aligned == [(":4*ag:5", "ABCDEFGHIJKLMNO", 2, 3), (":5+II:5", "abcdefghijkl", 0, 0), (":6", "MNOPQRS", 1, 0)]
    assert unmapped == ["!!~~"]
    aligned, unmapped = characterize.quals_from_sam(str(sam), primary_only=False)
    assert [a[0] for a in aligned] == [":4*ag:5", ":5+II:5", ":6", ":6"] and aligned[2] == (":6", "LLLLLLLL", 0, 2)
    sam.write_text(rec("noqual", 0, "4M", "*", "cs:Z::4"))
    with pytest.raises(ValueError, match="QUAL"):
        characterize.quals_from_sam(str(sam))
    sam.write_text(rec("notag", 0, "4M", "IIII"))
    with pytest.raises(ValueError):
        characterize.quals_from_sam(str(sam))


def test_written_file_loads_as_the_fastq_model(fx, host, tmp_path):
    """round trip: the file base_qualities writes, in place of the one of the small test model, is what load_model(fastq=True) reads"""
    dst = tmp_path / "model"
    shutil.copytree(os.path.join(ROOT, "tests", "golden", "model_small"), str(dst))
    prefix = str(dst / "training")
    t = characterize.base_qualities(prefix, fx["alignments"], fx["unmapped"], host)
    assert np.array_equal(t["hist"], fx["hist"])
    same_file(open(prefix + "_base_qualities_model_parameters.tsv").read(), fx["file"])
    m = model.load_model(prefix, fastq=True)
    fit = characterize.fit_qualities(fx["hist"])
    for name in TYPES:
        assert m.quals[name] == (fit[name][0], 0.0, fit[name][2])
    assert m.qual_thr.shape[0] == len(model.NS_Q_NAMES)


def test_struct_mirrors_match_the_header():
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "nanosim_amd.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu\n", sizeof(ns_qual_aln), offsetof(ns_qual_aln, head), offsetof(ns_qual_aln, tail), offsetof(ns_qual_aln, unmapped), offsetof(ns_qual_aln, reserved));
  printf("%zu %zu %zu %zu %zu\n", sizeof(ns_qual_hist), offsetof(ns_qual_hist, hist), offsetof(ns_qual_hist, n_short), offsetof(ns_qual_hist, n_bad_qual), offsetof(ns_qual_hist, ms_kernel));
  return 0; }'''
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
        sizes = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    A, H = characterize.NsQualAln, characterize.NsQualHist
    assert sizes[:5] == [C.sizeof(A), A.head.offset, A.tail.offset, A.unmapped.offset, A.reserved.offset]
    assert sizes[5:] == [C.sizeof(H), H.hist.offset, H.n_short.offset, H.n_bad_qual.offset, H.ms_kernel.offset]
    assert characterize.QUAL_ALN_DTYPE.itemsize == C.sizeof(A) and [characterize.QUAL_ALN_DTYPE.fields[n][1] for n in ("head", "tail", "unmapped", "reserved")] == sizes[1:5]
    assert "ns_qual_histograms" in engine.EXPORTS
