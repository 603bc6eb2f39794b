"""-k / --KmerBias: the homopolymer filter of mutate_read (S:1920-1947) and mutate_homo (S:618-705), pinned by tape
replay against the reference (fixtures: tests/golden/reference_functions.json["homopolymer"], sampled reads at k = 5, and
tests/golden/reference_hp_edges.json.gz, hand-built inputs with injected draws at the branches sampled reads do not reach)."""
import copy
import ctypes as C
import gzip
import json
import os

import numpy as np
import pytest

from nanosim_amd import model as M
from tests import oracle_lib as O
from tests.test_oracle_pin import _run_mutate, decode_events, events_array, expected_events


def filter_events(L, conv, events, k):
    seg = np.frombuffer(conv.encode(), dtype=np.uint8).copy()
    ev = events_array(events)
    sh = C.c_int64(0)
    n = L.nso_hp_filter(seg.ctypes.data, len(seg), ev.ctypes.data, len(ev), k, C.byref(sh))
    kept = decode_events(ev[:n])
    assert sh.value == sum(l if t == 1 else -l if t == 2 else 0 for _, t, l in kept)
    return kept


def test_hp_filter_and_mutate_read_match_reference(golden_functions):
    L = O.lib()
    names = ["mis", "ins", "del"]
    for case in golden_functions["homopolymer"]:
        kept = filter_events(L, case["converted"], expected_events(case["e_dict"]), case["k"])
        ref_rows = sorted((r[0], names.index(r[1]), r[2]) for r in case["log"])
        assert sorted(kept) == ref_rows                       # exactly the events the reference kept
        d, keep = O.make_tape(case["u_mutate"])
        out, cls, log = _run_mutate(L, case["converted"], kept, d)
        assert not d.tape_err and d.i_u == len(case["u_mutate"])
        assert out == case["out1"] and log == case["log"] and cls.tolist() == case["classes1"]


def test_survey_hand_case_with_k(golden_functions):
    L = O.lib()
    case = [c for c in golden_functions["mutate_read"] if c.get("k")][0]
    kept = filter_events(L, case["converted"], expected_events(case["e_dict"]), case["k"])
    d, keep = O.make_tape(case["u_mutate"])
    out, cls, log = _run_mutate(L, case["converted"], kept, d)
    assert out == case["out"] and log == case["log"] and len(out) == 30


def test_mutate_homo_tape_replay(golden_functions, small_model):
    L = O.lib()
    t = small_model.to_c()
    n_runs = 0
    for case in golden_functions["homopolymer"]:
        d, keep = O.make_tape(case["u_homo"], z=case["x_runs"])
        seq = np.frombuffer(case["out1"].encode(), dtype=np.uint8).copy()
        q = np.array(case["classes1"], dtype=np.uint8)
        out = np.zeros(2 * len(seq) + 64, dtype=np.uint8)
        oq = np.zeros_like(out)
        n = L.nso_mutate_homo(C.byref(t), seq.ctypes.data, q.ctypes.data, len(seq), case["k"], C.byref(d), 0, 0,
                              out.ctypes.data, oq.ctypes.data, len(out))
        assert n == len(case["out2"])
        assert not d.tape_err and d.i_u == len(case["u_homo"]) and d.i_z == len(case["x_runs"])
        assert bytes(out[:n]).decode() == case["out2"]
        assert oq[:n].tolist() == case["classes2"]
        n_runs += len(case["x_runs"])
    assert n_runs > 100


@pytest.fixture(scope="module")
def golden_hp_edges():
    with gzip.open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_hp_edges.json.gz"), "rt") as f:
        return json.load(f)


# what each branch counter of the oracle (tests/oracle_lib.py HP_COUNTERS) stands for, for the assertion messages
HP_BRANCHES_HOMO = {
    "runs": "a re-sampled run", "grow": "a run that grows", "grow_15": "a run that grows by more than 15 bases (several insertions at one position)",
    "shrink": "a run that shrinks", "shrink_4095": "a run that shrinks by more than 4095 bases (the deletion is split)",
    "size0": "a run re-sampled to size 0", "l64": "a run of 64 bases or more", "l1024": "a run of 1024 bases or more",
    "l4096": "a run of more than 4095 bases", "at_start": "a run at the first base of the segment", "at_end": "a run at the last base of the segment",
    "mis2": "a run with two or more mismatches", "mis_appended": "a mismatch on an appended base",
    "mis_mid_ins": "a first mismatch on an appended base that is not the first letter of its 15-letter insertion",
    "edits3": "a run with more than 2 edits", "tie": "a draw exactly on n + 1/2", "adjacent": "two re-sampled runs adjacent in the input"}
HP_BRANCHES_FILTER = {
    "drop_mis": "a substitution dropped", "drop_ins": "an insertion dropped", "drop_del": "a deletion dropped",
    "keep_mis": "a substitution kept", "keep_ins": "an insertion kept", "keep_del": "a deletion kept",
    "ins_key_before": "an insertion dropped only because base pos - 1 lies in a run (float key pos - 1/2)",
    "ins_key_beyond": "an insertion dropped only because a base beyond pos lies in a run",
    "near_end": "an event tested within 16 bases of an end of the segment", "run_cut": "a run that the end of the segment cuts below k"}


def test_hp_edge_filter_and_mutate_read_match_reference(golden_hp_edges):
    """the filter at k = 2, 3, 5, 8, 9, 16, 17 on hand-made e_dicts: events that end exactly where a run starts and start exactly where
    it ends, insertions decided by their float key alone, events on the first and last base, runs cut by the ends of the read"""
    L = O.lib()
    names = ["mis", "ins", "del"]
    O.hp_counts()
    assert sorted({c["k"] for c in golden_hp_edges["filter"]}) == [2, 3, 5, 8, 9, 16, 17]
    for case in golden_hp_edges["filter"]:
        kept = filter_events(L, case["converted"], expected_events(case["e_dict"]), case["k"])
        ref_rows = sorted((r[0], names.index(r[1]), r[2]) for r in case["log"])
        assert sorted(kept) == ref_rows                       # exactly the events the reference kept
        d, keep = O.make_tape(case["u_mutate"])
        out, cls, log = _run_mutate(L, case["converted"], kept, d)
        assert not d.tape_err and d.i_u == len(case["u_mutate"])
        assert out == case["out1"] and log == case["log"] and cls.tolist() == case["classes1"]
    cnt = O.hp_counts()
    for name, what in HP_BRANCHES_FILTER.items():
        assert cnt[name] > 0, "the filter tapes do not reach: " + what


def test_hp_edge_mutate_homo_tape_replay(golden_hp_edges, small_model):
    """mutate_homo on hand-built sequences with injected draws: ties n + 1/2 (Python's round is half to even), -0.0 and negative draws,
    growth by 1 .. 500 bases, runs of 15 .. 65, 1100 and 4200 bases (the last re-sampled to 0), adjacent runs, N runs, runs on the first
    and the last base, at hp_mis_rate 0.03 and 0.5; the quality CLASS of every base as well (a contraction drops the FIRST qualities of
    the run, S:688-690; only the first mismatch takes the mis class, S:697-700)"""
    L = O.lib()
    O.hp_counts()
    assert sorted({c["k"] for c in golden_hp_edges["homo"]}) == [2, 3, 5, 8, 9, 16, 17]
    assert {c["hp_mis_rate"] for c in golden_hp_edges["homo"]} == {0.03, 0.5}
    for case in golden_hp_edges["homo"]:
        m = copy.deepcopy(small_model)
        m.hp_mis_rate = case["hp_mis_rate"]
        t = m.to_c()
        d, keep = O.make_tape(case["u_homo"], z=case["x_runs"])
        seq = np.frombuffer(case["out1"].encode(), dtype=np.uint8).copy()
        q = np.array(case["classes1"], dtype=np.uint8)
        out = np.zeros(len(case["out2"]) + 64, dtype=np.uint8)
        oq = np.zeros_like(out)
        n = L.nso_mutate_homo(C.byref(t), seq.ctypes.data, q.ctypes.data, len(seq), case["k"], C.byref(d), 0, 0,
                              out.ctypes.data, oq.ctypes.data, len(out))
        assert n == len(case["out2"])
        assert not d.tape_err and d.i_u == len(case["u_homo"]) and d.i_z == len(case["x_runs"])
        assert bytes(out[:n]).decode() == case["out2"]
        assert oq[:n].tolist() == case["classes2"]
    cnt = O.hp_counts()
    for name, what in HP_BRANCHES_HOMO.items():
        assert cnt[name] > 0, "the mutate_homo tapes do not reach: " + what
    assert cnt["edits_max"] > 6, "the mutate_homo tapes do not reach: more than 6 edits for one run"


def test_get_nd_par(golden_samplers, small_model):
    L = O.lib()
    t = small_model.to_c()
    for length, vals in golden_samplers["get_nd_par"].items():
        for base, (mi, si) in ((ord("A"), (0, 1)), (ord("T"), (2, 3)), (ord("C"), (4, 5)), (ord("G"), (6, 7))):
            assert L.nso_hp_mu(C.byref(t), base, int(length)) == pytest.approx(vals[mi], rel=1e-12)
            assert L.nso_hp_sigma(C.byref(t), base, int(length)) == pytest.approx(vals[si], rel=1e-12)
