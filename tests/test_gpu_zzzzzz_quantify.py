"""GPU parity of the training side's quantification ("Quantification: the EM in the reference's order"): ns_em_quantify
(k_em_estep, k_em_accum, k_em_stop of csrc/ns_train.h) against the same iteration compiled for the host and against what the REAL
src/get_primary_sam.py computed and wrote (tests/golden/reference_quantify.json.gz) — bit for bit: abundance, count, the whole diff
trace, the iteration count.  The random problems stay at or below 500 targets and 2 000 reads and include n_multi == 0 and targets with
exactly W - 1, W, W + 1 and more than 3 W contributions (W = 64, the chunk of em_fold)."""
import ctypes as C
import os

import numpy as np
import pytest

from nanosim_amd import characterize
from nanosim_amd import engine as EN
from tests.test_quantify import build_host_engine, check_direct, check_fold_problems, items_of, load_fixture, sam_file

pytestmark = pytest.mark.gpu
W = 64


@pytest.fixture(scope="module")
def fx():
    return load_fixture()


@pytest.fixture(scope="module")
def host():
    return build_host_engine()


@pytest.fixture(scope="module")
def eng():
    e = EN.Engine(0)
    yield e
    e.close()


def same_bits(got, want):
    assert got["n_iter"] == want["n_iter"] and got["n_nonfinite"] == want["n_nonfinite"] == 0
    for k in ("abundance", "count", "diff_trace"):
        assert got[k].tobytes() == want[k].tobytes(), k


def random_problem(seed: int) -> dict:
    """an em_problem from a seed: kinds by turns; seed % 5 == 0 has no multi-mapping item, seed % 5 == 1 the W-border targets"""
    rng = np.random.default_rng(1000 + seed)
    kind = "meta" if seed % 2 else "trans"
    n = int(rng.integers(1, 501)) if seed % 5 != 1 else int(rng.integers(9, 501))
    names = ["x%d" % i for i in range(n)]
    items = {}
    n_reads = int(rng.integers(1, 1400))
    p_multi = 0.0 if seed % 5 == 0 else float(rng.uniform(0.1, 0.9))
    lo = 8 if seed % 5 == 1 else 0                           # (the border targets take no other contribution)
    for i in range(n_reads):
        a = lo + int(rng.integers(0, n - lo) * rng.random())   # skewed to the first targets; the last ones often stay without a read
        cand = [names[a]]
        if rng.random() < p_multi:
            cand += [names[int(rng.integers(lo, n))] for _ in range(int(rng.integers(1, 7)))]
        s = int(rng.integers(0, 50))
        items[("q%d" % (i if rng.random() < 0.97 else i // 2), (s, s + int(rng.integers(1, 5000))))] = cand
    if seed % 5 == 1:
        for t, cnt in ((1, W - 1), (2, W), (3, W + 1), (4, 3 * W + 5), (5, 2 * W)):
            for j in range(cnt):
                items[("b%d_%d" % (t, j), (0, 100 + j))] = [names[t], names[6 + j % 2]]
    return characterize.em_problem(items, names, kind)


def test_gpu_fixture_problems(fx, eng, host):
    """the reference's doubles, iteration counts and printed lines — and the host build's bits on top"""
    for d in fx["direct"]:
        check_direct(eng, d)
        prob = characterize.em_problem(items_of(d["items"]), [t for t, _ in d["targets"]], d["kind"])
        g = characterize.em_call(eng, prob)
        same_bits(g, characterize.em_call(host, prob))
        assert g["ms_kernel"] > 0
        print("%s: %d iterations, %.3f ms" % (d["name"], g["n_iter"], g["ms_kernel"]))


def test_gpu_fold_patterns_of_the_stop_sum(eng, host):
    """em_fold's device branch (chunks of 64 terms through cross-lane reads, two ways to fold a chunk) where only k_em_stop meets mixed
    chunks: dabs[] non-zero at none, one, 20, 21 or all lanes of a chunk, at 1 .. 200 targets — against the plain-Python EM, and against
    the host build, whose fold is a plain loop: another text"""
    for name, prob, got in check_fold_problems(eng):
        same_bits(got, characterize.em_call(host, prob))


def test_gpu_random_problems_equal_the_host_build(eng, host):
    seen = set()
    for seed in range(20):
        prob = random_problem(seed)
        g, h = characterize.em_call(eng, prob), characterize.em_call(host, prob)
        same_bits(g, h)
        seen.add((prob["kind"], len(prob["keys"]) == 0))
        if seed % 5 == 1:
            assert np.bincount(prob["target"], minlength=8)[1:6].tolist() == [W - 1, W, W + 1, 3 * W + 5, 2 * W]
    assert seen >= {("meta", False), ("trans", False), ("trans", True), ("meta", True)}


def test_gpu_end_to_end_texts(fx, eng, tmp_path):
    prefix, path = os.path.join(str(tmp_path), "training"), sam_file(fx, tmp_path)
    e = fx["e2e"]["chimeric_meta"]
    characterize.chimeric(prefix, path, eng, quantify="meta", primary_sam=False, pickles=False)
    with open(prefix + "_chimeric_info") as f:
        assert f.read() == e["chimeric_info"]
    with open(prefix + "_quantification.tsv") as f:
        assert f.read() == e["tsv"]
    result, variation = characterize.quantify(prefix, path, eng, "meta", expected=fx["expected"])
    assert [[k, v.hex()] for k, v in result.items()] == e["abundance"] and [v.hex() for v in variation] == e["variation"]
    result, _ = characterize.quantify(prefix, path, eng, "trans")
    with open(prefix + "_quantification.tsv") as f:
        assert f.read() == fx["e2e"]["chimeric_trans_q"]["tsv"]
    refs, records, _, _ = characterize.chimeric_records(path)
    res = characterize.em_quantify(eng, characterize.quant_items_primary(records, refs), characterize.quant_targets(refs, "meta"), "meta")
    e = fx["e2e"]["primary_meta"]
    assert characterize.format_quantification("meta", res["result"]) == e["tsv"] and res["n_iter"] == e["n_iter"]
    assert characterize.iteration_lines("meta", res["diff_trace"], res["n_iter"]) == e["lines"]


def test_gpu_calls_interleaved_with_another_training_call(fx, eng, host):
    """the scoped scratch: two EM calls on one engine with another training call between them give the same bits"""
    d = [d for d in fx["direct"] if d["name"] == "trans_300"][0]
    prob = characterize.em_problem(items_of(d["items"]), [t for t, _ in d["targets"]], "trans")
    small = random_problem(3)
    first = characterize.em_call(eng, prob)
    spans, n_bad, _, _ = characterize.cigar_spans(eng, ["%dS%dM" % (i, 100 + i) for i in range(200)])
    assert n_bad == 0 and spans["qstart"].tolist() == list(range(200))
    other = characterize.em_call(eng, small)
    second = characterize.em_call(eng, prob)
    same_bits(first, second)
    same_bits(second, characterize.em_call(host, prob))
    same_bits(other, characterize.em_call(host, small))


def test_gpu_error_codes(eng):
    P, R = characterize.NsEmProblem(), characterize.NsEmResult()
    unique, ab, cnt, trace = np.array([5.0]), np.zeros(1), np.zeros(1), np.ones(100)
    P.n_targets, P.total, P.factor, P.max_iter, P.unique = 0, 5.0, 0.01, 100, unique.ctypes.data
    R.abundance, R.count, R.diff_trace = ab.ctypes.data, cnt.ctypes.data, trace.ctypes.data
    q = lambda: eng.L.ns_em_quantify(eng.ctx, C.addressof(P), C.addressof(R))
    assert q() == EN.NS_EINVAL and b"ns_em_quantify" in eng.L.ns_last_error(eng.ctx)
    P.n_targets, P.total = 1, 0.0
    assert q() == EN.NS_EINVAL
    P.total = 5.0
    assert q() == 0 and R.n_iter == 1 and ab[0] == 100.0 and cnt[0] == 5.0 and not trace.any()
