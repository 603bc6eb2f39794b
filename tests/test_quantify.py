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
1, 63, 64, 65 and 300 targets; a transcript whose count prints as an int; problems without a multi-mapping item and with an unexpressed
target, which end through `0.0 <= 0.0`; one problem per kind run with the reference's iteration limit cut to 1, 2 and 3.  Of every
problem it holds the whole trace (every diff_tmp) and the minimum of every iteration.

The stop rule (em_decide) is also pinned alone: a transcription of G:81-84, replayed over those traces, gives the expected values for
a table of states at and next to the ties of both conditions.  py_em is the whole loop transcribed; the fold problems place the
targets that keep moving at chosen lanes of em_fold's chunks (the GPU file runs them on the device)."""
import contextlib
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
    """tests/em_host.cpp: -> (ns_em_quantify of the engine compiled for the host, em_decide alone)"""
    out = os.path.join(ROOT, "tests", "_tmp")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libem_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tests", "em_host.cpp")])
    L = C.CDLL(so)
    L.em_host_quantify.restype = C.c_int
    L.em_host_quantify.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.em_host_decide.restype = None
    L.em_host_decide.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_uint64, C.c_double, C.c_uint32, C.c_void_p]
    return L.em_host_quantify, L.em_host_decide


def build_host_engine():
    """stands in for an Engine: the chimeric walk and the EM, both compiled for the host; `em_decide` is the stop rule alone"""
    h = test_chimeric_train.build_host_walk()
    h.L.ns_em_quantify, h.em_decide = build_host_em()
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


@contextlib.contextmanager
def iteration_limit(kind, max_iter):
    """the calls inside run with the reference's `range(0, 100)` / `range(0, 1000)` cut to max_iter (None: as it is), as the fixture's
    *_max_iter_* problems were run"""
    was = characterize.EM_KINDS[kind]
    if max_iter is not None:
        characterize.EM_KINDS[kind] = (max_iter,) + was[1:]
    try:
        yield
    finally:
        characterize.EM_KINDS[kind] = was


def check_direct(eng, d):
    """one directly run EM problem against what the reference returned and printed; -> em_quantify's result"""
    items, targets = items_of(d["items"]), {t: v for t, v in d["targets"]}
    with iteration_limit(d["kind"], d["max_iter"]):
        got = characterize.em_quantify(eng, items, targets, d["kind"], d["normalize"]) if d["kind"] == "trans" else characterize.em_quantify(eng, items, targets, "meta")
        assert len(got["diff_trace"]) == (d["max_iter"] or characterize.EM_KINDS[d["kind"]][0])
    assert got["n_iter"] == d["n_iter"], d["name"]
    # the WHOLE trace, every double of it: the reference's diff_tmp of every iteration (the printed lines show every 10th or 50th)
    assert [float(v).hex() for v in got["diff_trace"][:got["n_iter"]]] == d["trace"], d["name"]
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
    # the edges of the stop rule (make_quantify_golden.py: edge_problems)
    by_name = {d["name"]: d for d in fx["direct"]}
    for kind in ("meta", "trans"):
        z = by_name[kind + "_zero_diff"]                       # `diff_tmp <= diff_thres` with 0.0 <= 0.0
        assert z["n_iter"] == 2 and z["trace"][1] == (0.0).hex() and z["mins"][1] == (0.0).hex() and z["branch"] == "le" and not z["multi_keys"]
        for k in (1, 2, 3):                                   # the limit ends the loop, and its last iteration still leaves its trace entry
            m = by_name["%s_max_iter_%d" % (kind, k)]
            assert m["max_iter"] == m["n_iter"] == len(m["trace"]) == k and m["branch"] is None and float.fromhex(m["trace"][-1]) > 0
        assert by_name[kind + "_max_iter_3"]["trace"][:2] == by_name[kind + "_max_iter_2"]["trace"]


# ---- the stop rule alone -------------------------------------------------------------------------------------------------------------------------
def ref_decide(diff, diff_tmp, abundance_min, factor):
    """G:81-84 (G:124-127), the three lines behind `abundance_list = abundance_list_tmp`, transcribed: -> (the loop breaks, diff afterwards)"""
    diff_thres = abundance_min * factor
    if diff_tmp <= diff_thres or diff - diff_tmp < diff_thres:
        return True, diff
    diff = diff_tmp
    return False, diff


def ref_iteration(diff, it, diff_tmp, abundance_min, factor, max_iter):
    """... inside `for iter in range(0, max_iter)`: -> (diff afterwards, iterations run so far, the loop is over)"""
    brk, diff = ref_decide(diff, diff_tmp, abundance_min, factor)
    return diff, it + 1, brk or it + 1 >= max_iter


def py_em(prob, max_iter=None):
    """G:60-84 (G:104-127) transcribed over an em_problem, every sum a left fold in the reference's order, Python floats being doubles:
    -> abundance, count, trace (lists), n_iter and `moving`: per iteration, the indices of the non-zero terms of the stop rule's sum.
    Shares no text with ns_em.h; test_python_em_equals_the_reference pins it."""
    limit, factor, _ = characterize.EM_KINDS[prob["kind"]]
    limit = max_iter or limit
    n, off, target, weight = len(prob["names"]), prob["multi_off"].tolist(), prob["target"].tolist(), prob["weight"].tolist()
    a = [100 / n] * n
    diff, trace, moving = 100 * n, [], []
    for it in range(limit):
        cnt = list(prob["unique_int"])
        for m in range(len(off) - 1):
            cand = target[off[m]:off[m + 1]]
            tot = 0
            for c in cand:
                tot = tot + a[c]
            for c in cand:
                cnt[c] += weight[m] * (a[c] / tot)
        new = [c * 100 / prob["total"] for c in cnt]
        d = 0
        for t in range(n):
            d = d + abs(new[t] - a[t])
        moving.append([t for t in range(n) if new[t] != a[t]])
        trace.append(d)
        a = new
        brk, diff = ref_decide(diff, d, min(a), factor)
        if brk:
            break
    return dict(abundance=a, count=[float(c) for c in cnt], trace=[float(d) for d in trace], n_iter=len(trace), moving=moving)


def same_as_py_em(got, want):
    """an em_call result against py_em's, double for double"""
    assert got["n_iter"] == want["n_iter"] and got["n_nonfinite"] == 0
    assert got["diff_trace"][:got["n_iter"]].tobytes() == np.array(want["trace"]).tobytes() and not got["diff_trace"][got["n_iter"]:].any()
    assert got["abundance"].tobytes() == np.array(want["abundance"]).tobytes() and got["count"].tobytes() == np.array(want["count"]).tobytes()


def test_python_em_equals_the_reference(fx, host):
    for d in fx["direct"]:
        if d["normalize"] is False:
            continue
        prob = characterize.em_problem(items_of(d["items"]), [t for t, _ in d["targets"]], d["kind"])
        want = py_em(prob, d["max_iter"])
        assert want["n_iter"] == d["n_iter"] and [v.hex() for v in want["trace"]] == d["trace"], d["name"]
        if d["kind"] == "meta":
            assert [v.hex() for v in want["abundance"]] == [r[1] for r in d["result"]], d["name"]
        else:
            assert [v.hex() for v in want["count"]] == [r[2] for r in d["result"]], d["name"]


# Where the terms of the stop rule's sum are not zero.  A target in no multi-mapping list stops moving after the second iteration, so from
# then on dabs[] is non-zero exactly at the targets of the lists: the patterns below place them inside the 64-term chunks of em_fold —
# none, one at lane 0, one at lane 63, exactly NS_EM_DENSE = 20 and 21 in a chunk (the two ways a chunk is folded), all 64, 21 followed by
# a chunk with none.  A ring does not keep every target of it moving for long, and not at every size: check_fold_problems counts what the
# iterations really show and asks for each pattern somewhere.
FOLD_SIZES = (1, 63, 64, 65, 128, 129, 200)
FOLD_PATTERNS = {"none": [], "lane 0": [0, 64], "lane 63": [63, 127], "lanes 0 and 63": [0, 63], "20": list(range(0, 60, 3)), "21": list(range(0, 63, 3)),
                 "all 64": list(range(64)), "21 then none": list(range(1, 64, 3)), "21 in the second chunk": list(range(64, 127, 3)),
                 "20 and 21": list(range(0, 60, 3)) + list(range(65, 128, 3)), "the last chunk's only term": [0, 199]}


def fold_problems():
    """[(name, em_problem)]: every pattern that fits, at every size; kinds by turns"""
    out = []
    for n in FOLD_SIZES:
        for k, (name, lanes) in enumerate(FOLD_PATTERNS.items()):
            if lanes and lanes[-1] >= n:
                continue
            names = ["t%d" % i for i in range(n)]
            items = {("u%d" % t, (0, 200 + 7 * (t % 13))): [names[t]] for t in range(n) if t % 5 != 3 or n == 1}       # (every fifth target has no read)
            for i, t in enumerate(lanes):                                     # a ring over the pattern, uneven: every target of it in two lists or more
                nxt = names[lanes[(i + 1) % len(lanes)]]
                items[("m%d" % i, (0, 300 + 37 * i))] = [names[t], nxt]
                if i % 2 == 0:
                    items[("d%d" % i, (0, 150 + i))] = [names[t], nxt, nxt]
                for j in range(i % 3):
                    items[("x%d_%d" % (i, j), (0, 90))] = [names[t]]
            out.append(("%d targets, %s" % (n, name), characterize.em_problem(items, names, "meta" if (k + n) % 2 else "trans")))
    return out


def check_fold_problems(eng):
    """em_call on every fold problem against py_em; -> [(name, problem, result)]"""
    out = []
    seen = set()
    counts, alone, in_a_row = set(), set(), set()              # what the chunks of dabs[] held, over every iteration of every problem
    for name, prob in fold_problems():
        got = characterize.em_call(eng, prob)
        want = py_em(prob)
        same_as_py_em(got, want)
        for moving in want["moving"]:
            per_chunk = [[t % 64 for t in moving if t // 64 == c] for c in range((len(prob["names"]) + 63) // 64)]
            counts.update(len(c) for c in per_chunk)
            alone.update(c[0] for c in per_chunk if len(c) == 1)
            in_a_row.update((len(a), len(b)) for a, b in zip(per_chunk, per_chunk[1:]))
        seen.add(name.split(", ")[1])
        out.append((name, prob, got))
        if "none" not in name:
            assert got["n_iter"] >= 3, name                                    # (iterations whose dabs[] shows the pattern were run)
    assert seen == set(FOLD_PATTERNS) and len(out) >= 40
    # none, one term (at lane 0, at lane 63), NS_EM_DENSE and one more, a full chunk; 21 with an empty chunk behind it, 20 with 21
    assert counts >= {0, 1, 20, 21, 64} and alone >= {0, 63} and in_a_row >= {(21, 0), (20, 21)}, (sorted(counts), sorted(alone), sorted(in_a_row))
    return out


def test_host_build_on_the_fold_patterns(host):
    check_fold_problems(host)


def test_transcribed_stop_rule_against_the_reference_traces(fx):
    """ref_decide replayed over what the reference itself summed and took the minimum of, iteration by iteration: it has to break where
    the reference broke and nowhere else — for every fixture problem, the ones that end through either condition or through the limit"""
    ended = set()
    for d in fx["direct"]:
        limit, factor, _ = characterize.EM_KINDS[d["kind"]]
        limit = d["max_iter"] or limit
        diff, it, over = 100 * len(d["targets"]), 0, False
        for t, mn in zip(d["trace"], d["mins"]):
            assert not over, d["name"]
            brk, _ = ref_decide(diff, float.fromhex(t), float.fromhex(mn), factor)
            diff, it, over = ref_iteration(diff, it, float.fromhex(t), float.fromhex(mn), factor, limit)
        assert over and it == d["n_iter"] and brk == (d["branch"] is not None), d["name"]
        ended.add(d["branch"])
    assert ended == {"le", "shrink", None}


def decide_table():
    """(diff, diff_tmp, min, factor): both conditions of G:82 one ulp below, at and one ulp above equality, with a threshold of 0 too"""
    up, down = lambda x: float(np.nextafter(x, np.inf)), lambda x: float(np.nextafter(x, -np.inf))
    rows = []
    for mn, factor in ((200.0, 0.01), (37.5, 0.001), (1e-3, 0.01), (0.0, 0.01), (0.0, 0.001)):
        th = mn * factor
        for diff_tmp in (th, up(th), down(th)) if th else (0.0, 5e-324, 1e-17):
            for diff in (300.0, diff_tmp, up(diff_tmp), down(diff_tmp) if diff_tmp else 0.0):
                rows.append((diff, diff_tmp, mn, factor))                   # the first condition at its edge, the second far off or at 0
        for diff_tmp in (8.0, 0.75, 1e-9 + 3 * th):
            tie = diff_tmp + th                                             # diff - diff_tmp == th where the sum is exact ...
            for diff in (tie, up(tie), down(tie), up(up(tie)), down(down(tie))):
                rows.append((diff, diff_tmp, mn, factor))                   # (... the neighbours cover it where it is not)
    return rows


def test_em_decide_table(host):
    """em_decide (ns_em.h) state by state against the transcription of G:80-84: the trace entry, the decision, diff and the count — at
    the ties of both conditions and at the first, the last but one and the last iteration of the limit"""
    decide = host.em_decide
    rows = decide_table()
    ties = {"le": 0, "shrink": 0}
    n = 0
    for diff, diff_tmp, mn, factor in rows:
        th = mn * factor
        ties["le"] += diff_tmp == th
        ties["shrink"] += diff - diff_tmp == th and diff_tmp > th
        for it, max_iter in ((0, 1), (0, 2), (1, 2), (1, 3), (2, 3), (0, 100), (97, 100), (98, 100), (99, 100), (998, 1000), (999, 1000)):
            want_diff, want_it, want_over = ref_iteration(diff, it, diff_tmp, mn, factor, max_iter)
            trace = np.full(max_iter + 1, -7.0)
            d, i, stop = C.c_double(diff), C.c_uint32(it), C.c_uint32(0)
            decide(C.addressof(d), C.addressof(i), C.addressof(stop), diff_tmp, mn, 0, factor, max_iter, trace.ctypes.data)
            assert (d.value.hex(), i.value, bool(stop.value)) == (float(want_diff).hex(), want_it, want_over), (diff, diff_tmp, mn, factor, it, max_iter)
            want_trace = np.full(max_iter + 1, -7.0)
            want_trace[it] = diff_tmp                                       # every iteration the loop runs leaves its entry, the last one too
            assert trace.tobytes() == want_trace.tobytes(), (it, max_iter)
            n += 1
    assert ties["le"] >= 5 and ties["shrink"] >= 5 and n == 11 * len(rows)
    # a value that is not finite ends the loop (the reference would run on and write `nan`; the caller raises)
    d, i, stop, trace = C.c_double(300.0), C.c_uint32(0), C.c_uint32(0), np.zeros(100)
    decide(C.addressof(d), C.addressof(i), C.addressof(stop), 50.0, 1.0, 1, 0.01, 100, trace.ctypes.data)
    assert stop.value == 1 and i.value == 1


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
