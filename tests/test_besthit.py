"""Training side, MAF input ("MAF input: the best hit per read") on CPU: the engine's line test, field parser and name table
(nanosim_amd/csrc/ns_maf_best.h, compiled for the host with the table operations run serially; on the GPU the k_maf_* kernels of
ns_train.h run it) and the host module around the call — pinned against what the REAL src/get_besthit_maf.py (besthit_and_unaligned)
wrote and returned for the same LAST file and reads file (tests/golden/reference_besthit.json.gz, tests/golden/make_besthit_golden.py),
and against hand-made inputs with their expectations written out."""
import ctypes as C
import gzip
import json
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest

from nanosim_amd import characterize, engine, model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDERS = {"file": 0, "reversed": 1, "shuffled": 2}


def load_fixture():
    with gzip.open(os.path.join(ROOT, "tests", "golden", "reference_besthit.json.gz"), "rt") as f:
        return json.load(f)


@pytest.fixture(scope="module")
def fx():
    return load_fixture()


def build_host_walk():
    """an object that stands in for an Engine: its ns_maf_besthit is the engine's per-thread code compiled for the host
    (tests/maf_best_host.cpp), its ns_maf_histograms the walk of tests/cs_hist_host.cpp behind the library's signature; `order(k)` sets
    the order in which the pairs visit the table, `span` is MAF_LINE_SPAN"""
    out = os.path.join(ROOT, "tests", "_tmp")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libmaf_best_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tests", "maf_best_host.cpp")])
    L = C.CDLL(so)
    L.maf_host_besthit.restype = C.c_int
    L.maf_host_besthit.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    L.maf_host_line_span.restype = C.c_uint64
    so = os.path.join(out, "libcs_hist_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tests", "cs_hist_host.cpp")])
    H = C.CDLL(so)
    H.maf_host_count.restype = C.c_int
    H.maf_host_count.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32] + [C.c_void_p] * 5

    def maf_histograms(ctx, ref, qry, nbytes, off, n, href):
        h = href._obj
        misc = np.zeros(4, dtype=np.uint64)
        H.maf_host_count(ref, qry, off, n, h.cap_match2d, C.addressof(h.dic), h.match_list, C.addressof(h.error_list), C.addressof(h.first_error),
                         misc.ctypes.data)
        h.max_match, h.n_match2d_overflow, h.n_skip = int(misc[0]), int(misc[1]), int(misc[2])
        return 0

    def check(rc):
        if rc:
            raise engine.EngineError("host walk: error %d" % rc)
    return types.SimpleNamespace(ctx=None, _check=check, order=L.maf_host_set_order, span=int(L.maf_host_line_span()),
                                 L=types.SimpleNamespace(ns_maf_besthit=L.maf_host_besthit, ns_maf_histograms=maf_histograms))


@pytest.fixture(scope="module")
def host():
    return build_host_walk()


def write_inputs(fx, tmp_path, maf=None, reads=None):
    paths = []
    for name, text in (("last.maf", fx["maf"] if maf is None else maf), ("reads.fasta", fx["reads"] if reads is None else reads)):
        paths.append(os.path.join(str(tmp_path), name))
        with open(paths[-1], "wb") as f:
            f.write(text.encode() if isinstance(text, str) else text)
    return paths


def same_figures(a, b):
    assert set(a) == set(b)
    for k in a:
        if k != "ms_kernel":
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k


def check_fixture(eng, fx, tmp_path, maf=None):
    """everything the reference wrote and returned for the fixture's input (or for `maf`, a text with the same `s` lines), exactly;
    -> besthit's dict"""
    maf_path, reads_path = write_inputs(fx, tmp_path, maf)
    prefix = os.path.join(str(tmp_path), "training")
    got = characterize.besthit(eng, maf_path, reads_path)
    characterize.write_besthit(prefix, maf_path, got)
    with open(prefix + "_besthit.maf", "rb") as f:
        assert f.read().decode() == fx["besthit"]
    assert got["unaligned_length"].dtype == np.int64 and got["unaligned_length"].tolist() == fx["unaligned_len"]
    assert got["strandness"] == fx["strandness"] and got["num_aligned"] == fx["n_names"] == len(got["lines"])
    assert got["pos_strand"] == sum(1 for r, q in zip(*[iter(fx["besthit"].splitlines())] * 2) if r.split()[4] == q.split()[4])
    same_figures(got["figures"], characterize.length_figures_maf(prefix + "_besthit.maf"))
    same_figures(characterize.figures_from_rows(got["figure_rows"], "transcriptome"), characterize.length_figures_maf(prefix + "_besthit.maf", "transcriptome"))
    same_figures(characterize.besthit(eng, maf_path, mode="transcriptome")["figures"], characterize.length_figures_maf(prefix + "_besthit.maf", "transcriptome"))
    assert got["records"] == characterize.maf_records(prefix + "_besthit.maf")
    return got


@pytest.mark.parametrize("order", list(ORDERS))
def test_host_choice_reproduces_the_reference_in_any_visiting_order(fx, host, tmp_path, order):
    host.order(ORDERS[order])
    try:
        got = check_fixture(host, fx, tmp_path)
    finally:
        host.order(0)
    assert fx["n_pairs"] == 3019 and fx["n_names"] == 1194 and len(fx["unaligned_len"]) == 134 and fx["strandness"] == 794 / 1194
    assert got["lines"]["ref_begin"].tolist() == sorted(got["lines"]["ref_begin"].tolist())              # file order


def test_fixture_holds_the_cases_the_kernels_have_paths_for(fx):
    """(the maker asserts them on its input; here: on the text that is committed)"""
    maf, kept = fx["maf"], fx["besthit"]
    lines = maf.split("\n")
    s_lines = [x for x in lines if x.startswith("s ") or x.startswith("s\t")]
    q = [x.split() for x in s_lines[1::2]]
    names = [x[1] for x in q]
    assert len(s_lines) == 2 * fx["n_pairs"] and len(set(names)) == fx["n_names"]
    assert names.count("hot") == 1000 and names.count("single") == 1
    at = [i for i, n in enumerate(names) if n == "scattered"]
    assert len(at) == 4 and min(b - a for a, b in zip(at, at[1:])) > 256
    assert {"read1", "read10", "read1x"} <= set(names) and any(len(n) > 64 for n in names)
    tie = [(i, int(x[3])) for i, x in enumerate(q) if x[1] == "tie3"]
    top = [i for i, s in tie if s == max(s for _, s in tie)]
    assert len(top) == 3 and top[1] - top[0] > 64 and top[2] - top[1] > 256 and tie[0][0] < top[0]
    assert [int(x[3]) for x in q if x[1] == "nine_ten"] == [9, 10] and [int(x[3]) for x in q if x[1] == "zero"] == [0]
    assert {(r.split()[4], x[4]) for r, x in zip(s_lines[0::2], q)} == {("+", "+"), ("+", "-"), ("-", "-")}
    assert any("    " in x for x in s_lines) and any(x.startswith("s\t") for x in s_lines) and not maf.endswith("\n")
    assert any(x.startswith("#") for x in lines) and any(x.startswith("a ") for x in lines) and "" in lines
    assert sum(1 for x in s_lines if len(x) + 1 >= 60000) == 2
    reads = fx["reads"]
    assert "\n\n" in reads and re.search(r"^>chrOnlyRef\b", reads, re.M) and "chrOnlyRef" not in names and re.search(r"^>\S+ runid=", reads, re.M)
    kq = [x.split() for x in kept.splitlines()[1::2]]
    by = {x[1]: int(x[3]) for x in kq}
    assert by["nine_ten"] == 10 and by["tie3"] == 1234 and [x[4] for x in kq if x[1] == "tie3"] == [q[top[0]][4]] and q[top[0]][4] != q[top[1]][4]


def test_the_lines_only_file_and_sizes_around_the_line_kernels_span_give_the_same(fx, host, tmp_path):
    maf = fx["maf"]
    s_only = "".join(x for x in maf.splitlines(True) if x.startswith("s ") or x.startswith("s\t"))
    check_fixture(host, fx, tmp_path, s_only)                      # what the reference was handed
    span = host.span
    assert span == 16384 and len(maf) > 30 * span

    def padded(total_mod):
        pad = (total_mod - len(maf)) % span
        pad += span if pad < 2 else 0
        return "#" + "x" * (pad - 2) + "\n" + maf
    for d in (-1, 0, 1):                                           # the total size one below, at and one above a multiple of the span
        text = padded(d)
        assert len(text) % span == d % span
        check_fixture(host, fx, tmp_path, text)
    # an `s` line that begins on the first, the second and the last byte of a span: its '\n', or its `s` and its blank, lie across the border
    start = maf.index("\ns ", 20 * span) + 1
    for d in (0, 1, span - 1):
        pad = (d - start) % span
        pad += span if pad < 2 else 0
        text = "#" + "x" * (pad - 2) + "\n" + maf
        assert (start + pad) % span == d and text[start + pad:start + pad + 2] == "s "
        check_fixture(host, fx, tmp_path, text)


def raw(eng, text, names=None):
    r = characterize.besthit_call(eng, np.frombuffer(text.encode() if isinstance(text, str) else text, dtype=np.uint8), names)
    o = r["raw"]
    return r, (int(o.n_lines), int(o.n_pairs), int(o.n_kept), int(o.pos_strand))


TINY_1 = "s ref 5 4 + 100 ACGT\ns only 0 4 + 4 ACGT\n"
PAIRS_3 = ("s ref 5 4 + 100 ACGT\ns n1 0 4 + 9 ACGT\n", "s ref 9 3 + 100 ACG\ns n2 1 3 - 8 ACG\n", "s ref 2 5 - 100 AC-GT\ns n3 2 4 - 7 ACTGT\n")
TINY_3 = "".join(PAIRS_3)


def check_tiny(eng):
    r, counts = raw(eng, TINY_1, [b"only", b"other", b"ref"])      # 1 pair: a table of 2 slots
    assert counts == (2, 1, 1, 1) and r["found"].tolist() == [True, False, False]
    assert r["lines"].tolist() == [(0, 21, 21, 41)] and r["figure_rows"].tolist() == [(4, 100, 0, 4, 0)]
    assert r["records"].tolist() == [(2, 16, 36, 3, 4, 4, 5)]
    r, counts = raw(eng, TINY_1[:-1])                              # no '\n' at the end: the last line ends with the text
    assert counts == (2, 1, 1, 1) and r["lines"].tolist() == [(0, 21, 21, 40)] and r["records"].tolist() == [(2, 16, 36, 3, 4, 4, 5)]
    r, counts = raw(eng, TINY_3, [b"n3", b"n2", b"n1", b"n", b"n11", b""])        # 3 pairs of 3 names: 8 slots
    assert counts == (6, 3, 3, 2) and r["found"].tolist() == [True, True, True, False, False, False]
    assert r["figure_rows"].tolist() == [(4, 100, 0, 9, 5), (3, 100, 1, 8, 5), (5, 100, 2, 7, 3)]
    assert [TINY_3[a:b] + TINY_3[c:d] for a, b, c, d in r["lines"].tolist()] == list(PAIRS_3)
    r, counts = raw(eng, TINY_3 + TINY_3)                          # every name twice with equal sizes: the first of each
    assert counts == (12, 6, 3, 2) and r["lines"]["ref_begin"].tolist() == [0, len(PAIRS_3[0]), len(PAIRS_3[0] + PAIRS_3[1])] and r["found"] is None
    r, counts = raw(eng, "", [b"a"])                               # the empty input is valid and keeps nothing
    assert counts == (0, 0, 0, 0) and r["found"].tolist() == [False] and len(r["lines"]) == 0
    r, counts = raw(eng, "# a header\n\na score=3\nsx 1 2\n", [b"a"])
    assert counts == (0, 0, 0, 0) and r["found"].tolist() == [False]
    r, counts = raw(eng, "s")
    assert counts == (0, 0, 0, 0)


def test_tiny_tables_and_the_empty_input(host):
    for order in ORDERS.values():
        host.order(order)
        try:
            check_tiny(host)
        finally:
            host.order(0)


# a trailing '\r' (a file from elsewhere): split() drops it from the last field; the lines are written as they stand.  Not in the
# fixture: the reference reads in text mode and would write '\n' for '\r\n'.
CR = "s ref 5 4 + 100 ACGT\r\ns rd 0 4 + 4 ACGT\r\ns ref 7 4 + 100 ACGA \r\ns rd 0 3 + 4 ACGA\r"


def check_carriage_returns(eng, tmp_path):
    maf_path, _ = write_inputs({}, tmp_path, CR, "")
    got = characterize.besthit(eng, maf_path)
    assert got["records"] == [("ref", 5, "ACGT", "ACGT")] and got["num_aligned"] == 1 and got["strandness"] == 1.0 and got["unaligned_length"] is None
    characterize.write_besthit(os.path.join(str(tmp_path), "cr"), maf_path, got)
    with open(os.path.join(str(tmp_path), "cr_besthit.maf"), "rb") as f:
        assert f.read() == b"s ref 5 4 + 100 ACGT\r\ns rd 0 4 + 4 ACGT\r\n"


def test_a_trailing_carriage_return_is_a_separator(host, tmp_path):
    check_carriage_returns(host, tmp_path)


BAD_LINES = ("s rd 0 42949672950 + 4 ACGT", "s rd x 4 + 4 ACGT", "s rd 0 4x + 4 ACGT", "s rd 0 4 + 4.0 ACGT", "s rd 0 +4 + 4 ACGT", "s rd 0 4294967296 + 4 ACGT", "s rd 0 4 + 99999999999999999999 ACGT",
             "s rd 0 4 + 4", "s rd", "s ", "s rd 0 -4 + 4 ACGT", "s rd 0 1_0 + 40 ACGT")
GOOD_LINES = ("s rd 0 4294967295 + 4294967295 ACGT", "s rd 0 4 + 4 ACGT extra words", "s  rd \t 00 \x0b 004 \x0c + 4 ACGT  ", "s rd 0 4 anything 4 ACGTT")


def check_value_errors(eng, tmp_path):
    good = "s ref 5 4 + 100 ACGT\n"

    def run(maf, reads=None):
        maf_path, reads_path = write_inputs({}, tmp_path, maf, reads or "")
        return characterize.besthit(eng, maf_path, reads_path if reads is not None else None)
    for bad in BAD_LINES:
        with pytest.raises(ValueError, match=r"last\.maf:5: not an `s` line"):
            run("# h\n" + TINY_1 + good + bad + "\n" + TINY_1)
        r, counts = raw(eng, TINY_1 + bad + "\n" + good)           # also as the reference line of a pair; nothing is counted
        assert counts == (4, 2, 0, 0) and (r["raw"].first_bad_line, r["raw"].first_bad_offset) == (2, 41)
    for ok in GOOD_LINES:
        assert run(TINY_1 + good + ok + "\n")["num_aligned"] == 2
    with pytest.raises(ValueError, match=r"last\.maf:4: an `s` line without its partner"):
        run("# h\n" + TINY_1 + good + "\n# the end\n")
    with pytest.raises(ValueError, match=r"last\.maf:1: an `s` line without its partner"):
        run(good[:-1])
    for nothing in ("", "# only a header\n", "a score=1\n\n"):
        with pytest.raises(ValueError, match="no alignment at all"):
            run(nothing)
    with pytest.raises(ValueError, match=r"last\.maf:3: .*reference sequence is the longer"):
        run(TINY_1 + "s ref 1 5 + 100 ACGTA\ns rd 0 4 + 4 ACGT\n")
    for head in (">\n", "> rd description\n", ">\t\n"):
        with pytest.raises(ValueError, match=r"reads\.fasta:3: a `>` header without a name"):
            run(TINY_1, ">only\nACGT\n" + head + "ACGT\n")
    with pytest.raises(ValueError, match=r"reads\.fasta:1: a sequence line in front of the first header"):
        run(TINY_1, "ACGT\n>only\nACGT\n")
    got = run(TINY_1, ">only x\nACGT\n>other\tdescription\nAC\n\n  ACG  \n>only\nA\n")
    assert got["unaligned_length"].tolist() == [2, 0, 3]
    assert run(TINY_1, "")["unaligned_length"].tolist() == [] and run(TINY_1)["unaligned_length"] is None


def test_every_value_error_and_the_lines_next_to_them(host, tmp_path):
    check_value_errors(host, tmp_path)


def test_reads_file_may_be_gzipped_and_besthit_and_unaligned_returns_the_references_pair(fx, host, tmp_path):
    maf_path, reads_path = write_inputs(fx, tmp_path)
    with gzip.open(reads_path + ".GZ", "wb") as f:
        f.write(fx["reads"].encode())
    with gzip.open(maf_path + ".gz", "wb") as f:
        f.write(fx["maf"].encode())
    prefix = os.path.join(str(tmp_path), "zipped")
    unaligned, strandness = characterize.besthit_and_unaligned(prefix, maf_path + ".gz", reads_path + ".GZ", host)
    assert unaligned.tolist() == fx["unaligned_len"] and strandness == fx["strandness"]
    with open(prefix + "_besthit.maf", "rb") as f:
        assert f.read().decode() == fx["besthit"]


def test_host_code_is_clean_under_the_sanitizers(fx, tmp_path):
    out = os.path.join(ROOT, "tests", "_tmp")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "maf_best_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DMAF_BEST_MAIN", "-o", exe,
                           os.path.join(ROOT, "tests", "maf_best_host.cpp")])
    maf_path, _ = write_inputs(fx, tmp_path)
    names = os.path.join(str(tmp_path), "names.txt")
    with open(names, "w") as f:
        f.write("\n".join(["hot", "ho", "hot_", "chrOnlyRef", "read1", "read1x", "read1y", "L" * 70, "L" * 70 + "a"]) + "\n")
    first, _ = subprocess.check_output([exe, maf_path, names], text=True).strip().split("\n")
    assert [int(v) for v in first.split()] == [2 * fx["n_pairs"], fx["n_pairs"], fx["n_names"], 794, 2 * fx["n_pairs"]]
    for k, text in enumerate((TINY_1, TINY_3, CR, "s", "s ", "s rd", "\ns\t", TINY_1 + "s ref 1 2", TINY_1[:-1], "")):
        p = os.path.join(str(tmp_path), "t%d.maf" % k)
        with open(p, "w", newline="") as f:
            f.write(text)
        subprocess.check_call([exe, p, names], stdout=subprocess.DEVNULL)


def test_struct_layout_export_and_abi():
    src = r'''#include <stdio.h>
#include <stddef.h>
#include "nanosim_amd.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(ns_maf_best_result), offsetof(ns_maf_best_result, found), offsetof(ns_maf_best_result, figures),
         offsetof(ns_maf_best_result, n_lines), offsetof(ns_maf_best_result, pos_strand), offsetof(ns_maf_best_result, first_bad_offset),
         offsetof(ns_maf_best_result, ms_kernel));
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(ns_maf_best_lines), sizeof(ns_maf_best_record), offsetof(ns_maf_best_record, ref_name_len),
         offsetof(ns_maf_best_record, ref_start), sizeof(ns_maf_best_figures), offsetof(ns_maf_best_figures, ht));
  printf("%u\n", NS_ABI_VERSION);
  return 0; }'''
    out = os.path.join(ROOT, "tests", "_tmp")
    os.makedirs(out, exist_ok=True)
    c = os.path.join(out, "maf_best_layout.c")
    with open(c, "w") as f:
        f.write(src)
    exe = os.path.join(out, "maf_best_layout")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, c])
    a, b, v = subprocess.check_output([exe], text=True).strip().split("\n")
    R = characterize.NsMafBestResult
    assert [int(x) for x in a.split()] == [C.sizeof(R), R.found.offset, R.figures.offset, R.n_lines.offset, R.pos_strand.offset, R.first_bad_offset.offset,
                                           R.ms_kernel.offset]
    rec, fig = characterize.MAF_RECORD_DTYPE, characterize.MAF_FIGURES_DTYPE
    assert [int(x) for x in b.split()] == [characterize.MAF_LINES_DTYPE.itemsize, rec.itemsize, rec.fields["ref_name_len"][1], rec.fields["ref_start"][1],
                                           fig.itemsize, fig.fields["ht"][1]] == [32, 40, 24, 36, 24, 16]
    assert "ns_maf_besthit" in engine.EXPORTS and int(v) == model.NS_ABI_VERSION == 7


def check_training(eng, fx, tmp_path):
    """train_genome_from_maf with model_fit=False next to a _model_profile from elsewhere: the prefix opens, its KDE arrays are the figures"""
    src = os.path.join(ROOT, "tests", "golden", "model_small")
    shutil.copy(os.path.join(src, "training_model_profile"), str(tmp_path / "training_model_profile"))
    maf_path, reads_path = write_inputs(fx, tmp_path)
    prefix = str(tmp_path / "training")
    got = characterize.train_genome_from_maf(prefix, maf_path, reads_path, eng, model_fit=False, pickles=False)
    with open(prefix + "_besthit.maf", "rb") as f:
        assert f.read().decode() == fx["besthit"]
    for suffix in ("_match.hist", "_mis.hist", "_ins.hist", "_del.hist", "_error_rate.tsv", "_error_markov_model", "_match_markov_model", "_first_match.hist",
                   "_kde.npz", "_strandness_rate", "_reads_alignment_rate"):
        assert os.path.getsize(prefix + suffix) > 0, suffix
    assert not os.path.exists(prefix + "_hp_lengths_model_parameters.tsv")
    assert open(prefix + "_strandness_rate").read() == "strandness:\t" + str(round(fx["strandness"], 3))
    assert open(prefix + "_reads_alignment_rate").read() == "Aligned / Unaligned ratio:\t" + str(fx["n_names"] * 1.0 / len(fx["unaligned_len"])) + "\n"
    m = model.load_model(prefix)
    fig = characterize.length_figures_maf(prefix + "_besthit.maf")
    for idx, data in ((model.NS_KDE_ALIGNED, fig["aligned_ref_length"].astype(np.float64)), (model.NS_KDE_HT, np.log10(fig["ht_length"] + 1)),
                      (model.NS_KDE_RATIO, fig["head_vs_ht_ratio"]), (model.NS_KDE_UNALIGNED, np.array(fx["unaligned_len"], dtype=np.float64))):
        assert np.array_equal(m.kde[idx][0], data), idx
    assert m.strandness_rate == round(fx["strandness"], 3)
    return got


def test_a_prefix_trains_from_a_maf_file_and_opens(fx, host, tmp_path):
    got = check_training(host, fx, tmp_path)
    # the histograms came from the kept pairs as the call returned them: the same as from the written file
    again = characterize.count_maf(host, characterize.maf_pairs(str(tmp_path / "training_besthit.maf")))
    first = characterize.count_maf(host, [(r, q) for _, _, r, q in got["records"]])
    assert np.array_equal(again["dic"], first["dic"]) and np.array_equal(again["error_list"], first["error_list"])
