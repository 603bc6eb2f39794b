"""Training side, the homopolymer-length model on CPU: the engine's walk over the two lines of a MAF alignment
(nanosim_amd/csrc/ns_hp_hist.h, compiled for the host; on the GPU the kernels of ns_train.h run it), the two fits and the host module around the call — pinned against what the REAL
src/model_homopolymer_lengths.py collected and wrote for the same alignments (tests/golden/reference_hp_train.json.gz,
tests/golden/make_hp_train_golden.py), against the `regex` module for the fuzzy match, and against a brute force for the piecewise
fit."""
import ctypes as C
import gzip
import itertools
import json
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

from nanosim_amd import characterize, engine, model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (1, 3, 5)
CLASSES = ("AT", "CG")


def load_fixture():
    with gzip.open(os.path.join(ROOT, "tests", "golden", "reference_hp_train.json.gz"), "rt") as f:
        fx = json.load(f)
    fx["records"] = [tuple(r) for r in fx["records"]]
    return fx


@pytest.fixture(scope="module")
def fx():
    return load_fixture()


def build_host_walk():
    """an object that stands in for an Engine: its ns_hp_histograms is the engine's walk compiled for the host (tests/hp_train_host.cpp)"""
    out = os.path.join(ROOT, "tests", "_tmp")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libhp_train_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tests", "hp_train_host.cpp")])
    L = C.CDLL(so)
    L.hp_host_histograms.restype = C.c_int
    L.hp_host_histograms.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    L.hp_host_fuzzy_len.restype = C.c_uint32
    L.hp_host_fuzzy_len.argtypes = [C.c_char_p, C.c_uint64, C.c_uint8]

    def check(rc):
        if rc:
            raise engine.EngineError("host walk: error %d" % rc)
    return types.SimpleNamespace(ctx=None, L=types.SimpleNamespace(ns_hp_histograms=L.hp_host_histograms), _check=check, fuzzy_len=L.hp_host_fuzzy_len)


@pytest.fixture(scope="module")
def host():
    return build_host_walk()


def expected_table(fx, k):
    """the reference's {class: {ref_len: [read_len ...]}} as the (2, R, Q) count table"""
    lengths = fx["k"][str(k)]["lengths"]
    R = max(x for c in CLASSES for x, _ in lengths[c]) + 1
    Q = max(v for c in CLASSES for _, ys in lengths[c] for v in ys) + 1
    t = np.zeros((2, R, Q), dtype=np.uint64)
    for ci, c in enumerate(CLASSES):
        for x, ys in lengths[c]:
            for v in ys:
                t[ci, x, v] += 1
    return t


def expected_columns(fx, k):
    """calc_homopolymer_mis_rate's four counters over the reference's span list (H:15-31)"""
    ins = dele = mis = match = 0
    for r, q, _ in fx["k"][str(k)]["spans"]:
        ins += r.count("-")
        dele += q.count("-")
        for a, b in zip(r, q):
            if a != "-" and b != "-":
                if a != b:
                    mis += 1
                else:
                    match += 1
    return [ins, dele, mis, match]


def spans_of(fx, records):
    """[reference part, read part, base] of every record (alignment, dash-less start, reference length, read length, base): the span
    begins at the first dash directly in front of the first letter unless the previous record's span reaches there, and ends behind
    the dashes that follow the last letter"""
    out, prev_aln, prev_end = [], -1, 0
    for aln, start, ref_len, _, base in records.tolist():
        ref, qry = fx["records"][aln][2], fx["records"][aln][3]
        if aln != prev_aln:
            prev_aln, prev_end = aln, 0
        cols = [i for i, c in enumerate(ref) if c != "-"]
        lo, hi = cols[start], cols[start + ref_len - 1] + 1
        while lo > prev_end and ref[lo - 1] == "-":
            lo -= 1
        while hi < len(ref) and ref[hi] == "-":
            hi += 1
        out.append([ref[lo:hi], qry[lo:hi], chr(base)])
        prev_end = hi
    return out


@pytest.mark.parametrize("k", KS)
def test_host_walk_equals_the_reference(fx, host, k):
    t = characterize.count_homopolymers(host, fx["records"], k, records=True)
    exp = expected_table(fx, k)
    assert t["table"].shape == exp.shape and np.array_equal(t["table"], exp)
    assert t["columns"].tolist() == expected_columns(fx, k)
    assert t["n_hp"] == len(fx["k"][str(k)]["spans"]) == len(t["records"])
    assert spans_of(fx, t["records"]) == fx["k"][str(k)]["spans"]
    # the read length of every record against the class tables' source: base and lengths, record by record
    rec = t["records"]
    got = np.zeros_like(exp)
    for _, _, ref_len, read_len, base in rec.tolist():
        got[0 if chr(base) in "AT" else 1, ref_len, read_len] += 1
    assert np.array_equal(got, exp)
    ins, dele, mis, match = t["columns"].tolist()
    assert mis / (dele + mis + match) == fx["k"][str(k)]["mis_rate"]
    assert characterize.fit_homopolymers(t["table"], t["columns"])["mis_rate"] == fx["k"][str(k)]["mis_rate"]


@pytest.mark.parametrize("k", (1, 5))
def test_host_walk_is_clean_under_the_sanitizers(fx, tmp_path, k):
    """the walk as a stand-alone program with -fsanitize=address,undefined (exact-size line buffers, the bounds of its local arrays) on
    the fixture's alignments; what it prints is the reference's: the number of spans and calc_homopolymer_mis_rate's four counters"""
    pairs = [(r[2], r[3]) for r in fx["records"] if r[2]]
    path = os.path.join(str(tmp_path), "pairs.txt")
    with open(path, "w") as f:
        f.write("".join("%s %s\n" % p for p in pairs))
    exe = os.path.join(str(tmp_path), "hp_train_host_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DHP_MAIN", "-o", exe,
                           os.path.join(ROOT, "tests", "hp_train_host.cpp")])
    out = subprocess.run([exe, path, str(k)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    got = [int(v) for v in out.stdout.split()]
    exp = expected_table(fx, k)
    assert got[:5] == [len(fx["k"][str(k)]["spans"])] + expected_columns(fx, k) and got[5:] == [exp.shape[1] - 1, exp.shape[2] - 1]


def test_fixture_holds_the_cases_the_kernel_has_paths_for(fx):
    lens = [len(r[2]) for r in fx["records"]]
    assert len(lens) > 256 + 64 and 0 in lens and max(lens) > 4096
    off = np.cumsum([0] + lens)[:-1]
    assert set(int(o) % 8 for o, n in zip(off, lens) if n) == set(range(8))
    t = expected_table(fx, 5)
    assert t.shape[1] > 256 and t.shape[2] > 256                       # beyond the LDS corner and beyond a first cap of 64
    assert t[:, :48, :48].sum() > 0.9 * t.sum()


def test_small_caps_overflow_and_retry(fx, host):
    full = characterize.count_homopolymers(host, fx["records"], 3, records=True)
    h = characterize.NsHpHist()
    table = np.zeros((2, 4, 4), dtype=np.uint64)
    h.cap_ref, h.cap_read, h.table = 4, 4, table.ctypes.data
    rb = b"".join(r[2].encode() for r in fx["records"])
    qb = b"".join(r[3].encode() for r in fx["records"])
    off = np.cumsum([0] + [len(r[2]) for r in fx["records"]]).astype(np.uint64)
    assert host.L.ns_hp_histograms(None, rb, qb, len(rb), off.ctypes.data, len(off) - 1, 3, C.byref(h)) == 0
    assert h.n_overflow == int(full["table"].sum() - full["table"][:, :4, :4].sum()) > 0
    assert h.max_ref == full["table"].shape[1] - 1 and h.max_read == full["table"].shape[2] - 1
    assert np.array_equal(table, full["table"][:, :4, :4])
    small = characterize.count_homopolymers(host, fx["records"], 3, records=True, cap_ref=2, cap_read=3, cap_records=5)
    assert np.array_equal(small["table"], full["table"]) and np.array_equal(small["records"], full["records"])


def test_fuzzy_read_length_equals_regex(host):
    regex = pytest.importorskip("regex", reason="the `regex` module (fuzzy matching) is not installed")
    pat = regex.compile("(AA+){s<=1}")
    n = 0
    for length in range(10):
        for tup in itertools.product("ACG", repeat=length):
            seg = "".join(tup)
            exp = 0
            for m in pat.finditer(seg):                                 # H:90-106
                s = m.group()
                v = len(s) - (s[0] != "A") - (s[-1] != "A")
                exp = max(exp, v)
            assert host.fuzzy_len(seg.encode(), len(seg), ord("A")) == exp, seg
            n += 1
    assert n == 29524


def test_fit_lr_equals_the_reference(fx, host):
    for k in KS:
        t = characterize.count_homopolymers(host, fx["records"], k)
        fit = characterize.fit_homopolymers(t["table"], t["columns"])
        for c in CLASSES:
            a, b = fx["k"][str(k)]["fit_lr"][c].split("\t")
            assert str(fit[c]["lr"][0]) == a == "0.0"
            assert fit[c]["lr"][1] == pytest.approx(float(b), rel=1e-12, abs=0)


def two_segments(x, const, alpha1, alpha2, psi):
    return const + alpha1 * x + (alpha2 - alpha1) * np.maximum(x - psi, 0.0)


@pytest.mark.parametrize("psi", [7.4, 9.0, 5.0, 13.0])
def test_fit_piecewise_recovers_noise_free_segments(psi):
    x = np.array([3, 4, 5, 6, 7, 8, 9, 10, 12, 13, 15, 16], dtype=np.float64)
    const, alpha1, alpha2 = 0.75, 0.9, 0.35
    got = characterize.fit_piecewise(x, two_segments(x, const, alpha1, alpha2, psi))
    assert got == pytest.approx((const, alpha2 - alpha1, psi, alpha1, alpha2), rel=1e-9, abs=1e-9)


def brute_force_rss(x, y):
    """the smallest residual sum over 10^4 breakpoints in [x[1], x[-2]], each a linear least-squares problem"""
    best = np.inf
    for psi in np.linspace(x[1], x[-2], 10000):
        A = np.stack([np.ones(len(x)), x, np.maximum(x - psi, 0.0)], axis=1)
        sol = np.linalg.lstsq(A, y, rcond=None)[0]
        r = y - A @ sol
        best = min(best, float(r @ r))
    return best


def test_fit_piecewise_is_not_worse_than_a_brute_force():
    rng = np.random.default_rng(12)
    for _ in range(50):
        n = int(rng.integers(4, 15))
        x = np.sort(rng.choice(np.arange(1, 40), n, replace=False)).astype(np.float64)
        y = two_segments(x, rng.normal(0, 1), rng.normal(1, 0.3), rng.normal(0.3, 0.3), rng.uniform(x[1], x[-2])) + rng.normal(0, 0.5, n)
        const, beta1, psi, alpha1, alpha2 = characterize.fit_piecewise(x, y)
        assert x[1] <= psi <= x[-2] and alpha2 == pytest.approx(alpha1 + beta1, rel=1e-15)
        r = y - two_segments(x, const, alpha1, alpha2, psi)
        bf = brute_force_rss(x, y)
        assert float(r @ r) <= bf * (1 + 1e-9)


def test_fit_needs_four_distinct_lengths_and_a_homopolymer():
    with pytest.raises(ValueError, match="did not converge"):
        characterize.fit_piecewise([5, 6, 7], [5.0, 5.5, 6.5])
    t = np.zeros((2, 12, 12), dtype=np.uint64)
    for x in (5, 6, 7):
        t[:, x, x] = 3
    with pytest.raises(ValueError, match="did not converge"):
        characterize.fit_homopolymers(t, [1, 1, 1, 100])
    with pytest.raises(ValueError, match="no homopolymer"):
        characterize.fit_homopolymers(np.zeros((2, 1, 1), dtype=np.uint64), [0, 0, 0, 0])


def write_files(eng, fx, k, tmp_path, name):
    prefix = str(tmp_path / name)
    characterize.homopolymer_lengths(prefix, fx["records"], eng, min_hp_len=k)
    return open(prefix + "_hp_lengths_model_parameters.tsv").read(), open(prefix + "_hp_lengths.tsv").read()


@pytest.mark.parametrize("k", KS)
def test_lengths_file_equals_the_reference(fx, host, tmp_path, k):
    assert write_files(host, fx, k, tmp_path, "training")[1] == fx["k"][str(k)]["lengths_file"]


def test_parameters_file_loads_through_the_simulators_loader(fx, host, tmp_path):
    import tests.oracle_lib as O
    src = os.path.join(ROOT, "tests", "golden", "model_small")
    for f in os.listdir(src):
        if os.path.isfile(os.path.join(src, f)):
            shutil.copy(os.path.join(src, f), str(tmp_path / f))
    text, _ = write_files(host, fx, 5, tmp_path, "training")
    lines = text.split("\n")
    assert lines[0] == "#Homopolymer mismatch rate: " + str(fx["k"]["5"]["mis_rate"])
    assert lines[1] == "base\tconst\tbeta1\tbreakpoint1\talpha1\talpha2\tintercept\tslope" and [l.split("\t")[0] for l in lines[2:4]] == ["AT", "CG"]
    t = characterize.count_homopolymers(host, fx["records"], 5)
    fit = characterize.fit_homopolymers(t["table"], t["columns"])
    m = model.load_model(str(tmp_path / "training"), chimeric=True, homopolymer=True, fastq=True)
    assert m.hp_mis_rate == fx["k"]["5"]["mis_rate"]
    tab = m.to_c()
    L = O.lib()
    for c, bases in (("AT", "AT"), ("CG", "CG")):
        const, beta1, psi, alpha1, alpha2 = fit[c]["pw"]
        assert m.hp[c]["betas"] == [beta1] and m.hp[c]["breakpoints"] == [psi] and m.hp[c]["const"] == const and m.hp[c]["alpha1"] == alpha1
        for length in range(5, 31):
            mu = const + alpha1 * length + beta1 * max(length - psi, 0.0)
            sigma = fit[c]["lr"][0] + fit[c]["lr"][1] * length
            for b in bases:
                assert L.nso_hp_mu(C.byref(tab), ord(b), length) == pytest.approx(mu, rel=1e-12)
                assert L.nso_hp_sigma(C.byref(tab), ord(b), length) == pytest.approx(sigma, rel=1e-12)


def test_min_hp_len_and_line_lengths(host):
    with pytest.raises(ValueError, match="min_hp_len"):
        characterize.count_homopolymers(host, [("AAAAA", "AAAAA")], 0)
    with pytest.raises(ValueError, match="differ in length"):
        characterize.count_homopolymers(host, [("AAAAA", "AAAA")], 1)
    with pytest.raises(ValueError, match="reference name"):
        characterize.homopolymer_lengths("unused", [("AAAAA", "AAAAA")], host)
    t = characterize.count_homopolymers(host, [], 5, records=True)
    assert t["table"].shape == (2, 1, 1) and not t["table"].any() and t["n_hp"] == 0 and t["records"].shape == (0, 5)
    t = characterize.count_homopolymers(host, [("", ""), ("", "")], 1, records=True)
    assert not t["table"].any() and not t["columns"].any() and t["records"].shape == (0, 5)


def test_maf_records_skips_headers_and_blank_lines(tmp_path):
    p = tmp_path / "x.maf"
    p.write_text("##maf version=1\n\na score=5\ns chr2 1200 6 + 5000 AAA-CCC\ns read1 0 7 + 7 AAATCCC\n\n"
                 "a score=7\ns\tchr1\t7\t3\t+\t5000\tGG-T\ns\tread2\t3\t4\t-\t9\tGGATTT\n")
    recs = characterize.maf_records(str(p))
    assert recs == [("chr2", 1200, "AAA-CCC", "AAATCCC"), ("chr1", 7, "GG-T", "GGAT")]
    assert characterize.maf_pairs(str(p)) == [r[2:] for r in recs]
    p.write_text("s chr2 1200 6 + 5000 AAA\n")
    with pytest.raises(ValueError, match="partner"):
        characterize.maf_records(str(p))


def test_struct_layout_and_export():
    src = r'''#include <stdio.h>
#include <stddef.h>
#include "nanosim_amd.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(ns_hp_hist), offsetof(ns_hp_hist, table), offsetof(ns_hp_hist, records),
         offsetof(ns_hp_hist, cap_records), offsetof(ns_hp_hist, n_hp), offsetof(ns_hp_hist, columns), offsetof(ns_hp_hist, max_ref),
         offsetof(ns_hp_hist, n_overflow), offsetof(ns_hp_hist, ms_kernel));
  printf("%zu\n", sizeof(ns_hp_record));
  return 0; }'''
    out = os.path.join(ROOT, "tests", "_tmp")
    os.makedirs(out, exist_ok=True)
    c = os.path.join(out, "hp_layout.c")
    with open(c, "w") as f:
        f.write(src)
    exe = os.path.join(out, "hp_layout")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, c])
    a, b = subprocess.check_output([exe], text=True).strip().split("\n")
    H = characterize.NsHpHist
    assert [int(v) for v in a.split()] == [C.sizeof(H), H.table.offset, H.records.offset, H.cap_records.offset, H.n_hp.offset, H.columns.offset,
                                           H.max_ref.offset, H.n_overflow.offset, H.ms_kernel.offset]
    assert int(b) == characterize.HP_RECORD_DTYPE.itemsize == 16
    assert "ns_hp_histograms" in engine.EXPORTS
