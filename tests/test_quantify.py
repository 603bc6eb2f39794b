"""Training side, quantification ("Quantification: the EM in the reference's order") on CPU: the engine's EM iteration
(nanosim_amd/csrc/ns_em.h, compiled for the host with -ffp-contract=off; on the GPU k_em_estep, k_em_accum and k_em_stop of ns_train.h
run it) and the host module around the call — pinned against what the REAL src/get_primary_sam.py (EM_meta, EM_trans,
primary_and_unaligned_chimeric, primary_and_unaligned) computed, printed and wrote (tests/golden/reference_quantify.json.gz,
tests/golden/make_quantify_golden.py).  Every double is compared by float.hex, the iteration count exactly, the diff trace at the
iterations the reference printed.

The fixture holds (make_quantify_golden.py asserts each): a trans problem of 300 transcripts with an unexpressed one (threshold 0) that
ends before iteration 1000 through `diff - diff_tmp < thres`; problems that end through `diff_tmp <= thres`; meta problems on which all
100 iterations run; one without a multi-mapping item; two with one target; both key collisions, a restarted list, lists with a
duplicate, of 2 and of >= 5 candidates; targets with exactly W - 1, W, W + 1 and 3 W + 9 contributions (W = 64, the chunk of em_fold);
1, 63, 64, 65 and 300 targets; a transcript whose count prints as an int."""
import ctypes as C
import gzip
import json
import os
import subprocess
import types

import numpy as np
import pytest

from nanosim_amd import characterize, engine
from tests import test_chimeric_train

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EM_QUANTIFY, EM_KINDS = characterize.em_quantify, characterize.EM_KINDS          # (the eighth piece: without it this module does not import)
assert "ns_em_quantify" in engine.EXPORTS


def load_fixture():
    with gzip.open(os.path.join(ROOT, "tests", "golden", "reference_quantify.json.gz"), "rt") as f:
        fx = json.load(f)
    fx["refs"] = [tuple(r) for r in fx["refs"]]
    return fx


def items_of(packed) -> dict:
    return {(q[0], (q[1], q[2])): list(q[3]) for q in packed}


def build_host_em():
    """ns_em_quantify of the engine compiled for the host (tests/em_host.cpp)"""
    out = os.path.join(ROOT, "tests", "_tmp")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libem_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tests", "em_host.cpp")])
    L = C.CDLL(so)
    L.em_host_quantify.restype = C.c_int
    L.em_host_quantify.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    return L.em_host_quantify


def build_host_engine():
    """stands in for an Engine: the chimeric walk and the EM, both compiled for the host"""
    h = test_chimeric_train.build_host_walk()
    h.L.ns_em_quantify = build_host_em()
    return h


@pytest.fixture(scope="module")
def fx():
    return load_fixture()


@pytest.fixture(scope="module")
def host():
    return build_host_engine()


def sam_file(fx, tmp_path):
    path = os.path.join(str(tmp_path), "training.sam")
    with open(path, "w") as f:
        f.write(fx["sam"])
    return path


def check_direct(eng, d):
    """one directly run EM problem against what the reference returned and printed; -> em_quantify's result"""
    items, targets = items_of(d["items"]), {t: v for t, v in d["targets"]}
    got = characterize.em_quantify(eng, items, targets, d["kind"], d["normalize"]) if d["kind"] == "trans" else characterize.em_quantify(eng, items, targets, "meta")
    assert got["n_iter"] == d["n_iter"], d["name"]
    assert characterize.iteration_lines(d["kind"], got["diff_trace"], got["n_iter"]) == d["lines"], d["name"]
    assert list(got["result"]) == [r[0] for r in d["result"]]
    for row in d["result"]:
        v = got["result"][row[0]]
        if d["kind"] == "meta":
            assert v.hex() == row[1], (d["name"], row[0])
        else:
            assert repr(v[0]) == row[1] and float(v[0]).hex() == row[2] and v[1].hex() == row[3], (d["name"], row[0])
    assert not got["diff_trace"][got["n_iter"]:].any()
    return got


def test_host_build_reproduces_the_reference_em(fx, host):
    assert fx["W"] == 64
    names = [d["name"] for d in fx["direct"]]
    assert sorted(set(len(d["targets"]) for d in fx["direct"])) == [1, 3, 63, 64, 65, 300]
    assert {d["branch"] for d in fx["direct"]} == {"le", "shrink", None}
    for d in fx["direct"]:
        got = check_direct(host, d)
        if d["name"] == "trans_300":
            assert got["n_iter"] < 1000 and d["branch"] == "shrink" and d["per_target"][100:104] == [63, 64, 65, 201]
            assert type(got["result"]["t9"][0]) is int and got["result"]["t9"][0] == 7 and type(got["result"]["t0"][0]) is float
            assert got["result"]["t5"][0] == 0 and got["result"]["t5"][1] == 0.0
        if d["name"] in ("meta_100_iterations", "meta_64"):
            assert got["n_iter"] == 100 and d["branch"] is None
    assert "meta_unique_only" in names and "trans_one" in names


def test_em_problem_against_the_reference_dictionaries(fx):
    for d in fx["direct"]:
        if d["normalize"] is False:
            continue
        p = characterize.em_problem(items_of(d["items"]), [t for t, _ in d["targets"]], d["kind"])
        keys = [list(k) if isinstance(k, tuple) else k for k in p["keys"]]
        assert keys == d["multi_keys"] and p["unique_int"] == d["unique"] and p["total"] == d["total"], d["name"]
        assert np.bincount(p["target"], minlength=len(p["names"])).tolist() == d["per_target"]
        assert int(p["multi_off"][-1]) == len(p["target"]) and len(p["weight"]) == len(p["keys"])
        if d["kind"] == "meta":
            assert p["weight"].tolist() == [float(k[1]) for k in p["keys"]]
    # the collisions, written out: the later list replaces the earlier one and keeps its place; total counts both
    p = characterize.em_problem({("r", (0, 400)): ["a", "b"], ("s", (0, 100)): ["a", "b"], ("r", (50, 450)): ["b", "c", "c"], ("r", (0, 7)): ["a"]}, ["a", "b", "c"], "meta")
    assert p["keys"] == [("r", 400), ("s", 100)] and p["target"].tolist() == [1, 2, 2, 0, 1] and p["total"] == 907 and p["unique_int"] == [7, 0, 0]
    p = characterize.em_problem({("r", (0, 400)): ["a", "b"], ("s", (0, 100)): ["a", "b"], ("r", (50, 451)): ["b", "c", "c"]}, ["a", "b", "c"], "trans")
    assert p["keys"] == ["r", "s"] and p["target"].tolist() == [1, 2, 2, 0, 1] and p["total"] == 3 and p["weight"].tolist() == [1.0, 1.0]


def test_quant_items_against_the_reference_dictionaries(fx, host, tmp_path):
    refs, records, _, _ = characterize.chimeric_records(sam_file(fx, tmp_path))
    species = {n: characterize.species_of_reference(n) for n, _ in refs}
    for key, sp in (("chimeric_meta", species), ("chimeric_trans_q", None)):
        sel = characterize.select_chimeric(host, refs, records, sp)
        got = characterize.quant_items(records, sel, refs, sp)
        want = items_of(fx["e2e"][key]["quant"])
        assert list(got.items()) == list(want.items()), key          # keys, lists and the ORDER of the dict
        assert list(characterize.quant_targets(refs, "meta" if sp else "trans", sp).items()) == [tuple(t) for t in fx["e2e"][key]["targets"]]
    got = characterize.quant_items_primary(records, refs)
    assert list(got.items()) == list(items_of(fx["e2e"]["primary_meta"]["quant"]).items())
    # the corners by name (make_quantify_golden.py: extra_reads)
    assert got[("restart", (10, 410))] == ["spB"] and got[("late", (0, 350))] == ["spA", "spB"] and got[("hardclip0", (0, 500))] == ["spA"]
    assert got[("eqxprimary", (5, 198))] == ["spA"] and got[("samelen", (25, 625))] == ["spA", "spB", "spA"]


def test_end_to_end_texts(fx, host, tmp_path):
    prefix = os.path.join(str(tmp_path), "training")
    path = sam_file(fx, tmp_path)
    # the reference's q_mode, both kinds: only _quantification.tsv is written
    e = fx["e2e"]["chimeric_meta"]
    result, variation = characterize.quantify(prefix, path, host, "meta", expected=fx["expected"])
    with open(prefix + "_quantification.tsv") as f:
        assert f.read() == e["tsv"]
    assert [[k, v.hex()] for k, v in result.items()] == e["abundance"] and [v.hex() for v in variation] == e["variation"]
    assert sorted(os.listdir(str(tmp_path))) == ["training.sam", "training_quantification.tsv"]
    e = fx["e2e"]["chimeric_trans_q"]
    result, variation = characterize.quantify(prefix, path, host, "trans")
    with open(prefix + "_quantification.tsv") as f:
        assert f.read() == e["tsv"] == characterize.format_quantification("trans", result)
    assert variation is None
    # the non-chimeric path
    e = fx["e2e"]["primary_meta"]
    refs, records, _, _ = characterize.chimeric_records(path)
    res = characterize.em_quantify(host, characterize.quant_items_primary(records, refs), characterize.quant_targets(refs, "meta"), "meta")
    assert characterize.format_quantification("meta", res["result"]) == e["tsv"] and res["n_iter"] == e["n_iter"]
    assert characterize.iteration_lines("meta", res["diff_trace"], res["n_iter"]) == e["lines"]
    assert [v.hex() for v in characterize.abundance_variation(res["result"], fx["expected"])] == e["variation"]


def test_chimeric_with_its_own_abundances(fx, host, tmp_path):
    """chimeric(quantify="meta"): _chimeric_info with the shrinkage rate from the EM's abundances, and _quantification.tsv"""
    prefix = os.path.join(str(tmp_path), "training")
    e = fx["e2e"]["chimeric_meta"]
    characterize.chimeric(prefix, sam_file(fx, tmp_path), host, quantify="meta", primary_sam=False, pickles=False)
    with open(prefix + "_chimeric_info") as f:
        assert f.read() == e["chimeric_info"]
    with open(prefix + "_quantification.tsv") as f:
        assert f.read() == e["tsv"]
    os.remove(prefix + "_quantification.tsv")
    characterize.chimeric(prefix, sam_file(fx, tmp_path), host, quantify="trans", primary_sam=False, pickles=False)
    with open(prefix + "_quantification.tsv") as f:
        assert f.read() == fx["e2e"]["chimeric_trans_q"]["tsv"]
    with open(prefix + "_chimeric_info") as f:
        assert f.read() == e["chimeric_info"].split("Shrinkage")[0]
    os.remove(prefix + "_quantification.tsv")
    characterize.chimeric(prefix, sam_file(fx, tmp_path), host, primary_sam=False, pickles=False)          # the default: as before
    assert not os.path.exists(prefix + "_quantification.tsv")


def test_error_cases(fx, host, tmp_path):
    with pytest.raises(ValueError):
        characterize.em_problem({("r", (0, 2 ** 53 // 100 + 1)): ["a"]}, ["a"], "meta")
    characterize.em_problem({("r", (0, 2 ** 53 // 100)): ["a"]}, ["a"], "meta")
    with pytest.raises(ValueError):
        characterize.em_problem({("r", (0, 5)): ["a", "zz"]}, ["a"], "meta")
    with pytest.raises(ValueError):
        characterize.em_problem({}, ["a"], "trans")
    with pytest.raises(ValueError):
        characterize.em_problem({("r", (0, 5)): ["a"]}, [], "trans")
    with pytest.raises(ValueError):
        characterize.em_problem({("r", (0, 5)): ["a"]}, ["a"], "genome")
    prefix, path = os.path.join(str(tmp_path), "training"), sam_file(fx, tmp_path)
    with pytest.raises(ValueError):
        characterize.quantify(prefix, path, host, "meta", expected={"spA": 100.0})          # spB of the header is missing
    with pytest.raises(ValueError):
        characterize.chimeric(prefix, path, host, quantify="meta", abundance={"spA": 50, "spB": 50})
    with pytest.raises(ValueError):
        characterize.chimeric(prefix, path, host, quantify="both")
    # n_nonfinite: a result that is not finite is an error, not a file
    fake = types.SimpleNamespace(ctx=None, _check=lambda rc: None, L=types.SimpleNamespace(
        ns_em_quantify=lambda ctx, p, r: C.cast(r, C.POINTER(characterize.NsEmResult)).contents.__setattr__("n_nonfinite", 2)))
    with pytest.raises(ValueError):
        characterize.em_quantify(fake, {("r", (0, 5)): ["a"]}, ["a"], "meta")
    # the C side: no target, no total
    q = host.L.ns_em_quantify
    P, R = characterize.NsEmProblem(), characterize.NsEmResult()
    unique, ab, cnt, trace = np.array([5.0]), np.zeros(1), np.zeros(1), np.ones(100)
    P.n_targets, P.total, P.factor, P.max_iter, P.unique = 0, 5.0, 0.01, 100, unique.ctypes.data
    R.abundance, R.count, R.diff_trace = ab.ctypes.data, cnt.ctypes.data, trace.ctypes.data
    assert q(None, C.addressof(P), C.addressof(R)) != 0
    P.n_targets, P.total = 1, 0.0
    assert q(None, C.addressof(P), C.addressof(R)) != 0
    P.total = 5.0
    assert q(None, C.addressof(P), C.addressof(R)) == 0 and R.n_iter == 1 and ab[0] == 100.0 and cnt[0] == 5.0 and not trace.any()


def test_struct_layouts_and_exports(tmp_path):
    src = os.path.join(str(tmp_path), "layout.c")
    with open(src, "w") as f:
        f.write('''#include <stdio.h>
#include <stddef.h>
#include "nanosim_amd.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(ns_em_problem), offsetof(ns_em_problem, n_targets), offsetof(ns_em_problem, n_multi),
         offsetof(ns_em_problem, multi_off), offsetof(ns_em_problem, target), offsetof(ns_em_problem, weight), offsetof(ns_em_problem, unique),
         offsetof(ns_em_problem, total), offsetof(ns_em_problem, factor), offsetof(ns_em_problem, max_iter), offsetof(ns_em_problem, group));
  printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(ns_em_result), offsetof(ns_em_result, abundance), offsetof(ns_em_result, count),
         offsetof(ns_em_result, diff_trace), offsetof(ns_em_result, n_iter), offsetof(ns_em_result, reserved), offsetof(ns_em_result, n_nonfinite),
         offsetof(ns_em_result, ms_kernel));
  return 0;
}
''')
    exe = os.path.join(str(tmp_path), "layout")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
    rows = [[int(v) for v in l.split()] for l in subprocess.check_output([exe]).decode().splitlines()]
    for row, S in zip(rows, (characterize.NsEmProblem, characterize.NsEmResult)):
        assert row == [C.sizeof(S)] + [getattr(S, n).offset for n, _ in S._fields_]
    assert "ns_em_quantify" in engine.EXPORTS
    with open(os.path.join(ROOT, "include", "nanosim_amd.h")) as f:
        assert "#define NS_ABI_VERSION 7u" in f.read()        # an added function, no ABI bump


def test_host_build_is_clean_under_the_sanitizers(tmp_path):
    """the iteration as a stand-alone program with -fsanitize=address,undefined (exact-size buffers: a slot or a candidate out of range is
    an error), with and without multi-mapping items, for both kinds"""
    exe = os.path.join(str(tmp_path), "em_host_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DEM_MAIN",
                           "-o", exe, os.path.join(ROOT, "tests", "em_host.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = out.stdout.splitlines()
    assert len(rows) == 4 and int(rows[0].split()[0]) >= 1 and rows[0].split()[1] == "0" and abs(float(rows[0].split()[2]) - 100.0) < 1e-9
