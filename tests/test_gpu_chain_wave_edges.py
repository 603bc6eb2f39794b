"""GPU side of tests/test_chain_wave64.py: what the engine can be steered to of the wave-per-read lists' edges, in batches of 16-64 reads
against the oracle.  The first test needs no GPU and runs with the CPU suite: it asserts, from the traces of test_chain_wave64 and the
oracle's output alone, that the batches contain what they are for — a dict-key collision at block-local index 0 of coop_error_list,
attempts dropped for `range`, reads that ask the 17th match-length column, run lengths of 65 536.

  - the zero-match hand model with every read on coop_error_list (NS_COOP_MIN=1, NS_COOP_SHIFT=0);
  - an unaligned batch on insertion tables of 1 365 entries (three merged insertions fit an event, four do not; ninety-six overflow the
    shift): the redraws the oracle makes are the redraws the engine counts, with K iterations per lane and with one (NS_UCOOP_K=1);
  - 16 match-length columns, the most coop_error_list holds, and 17, which ns_coop_ok (ns_pack.h) must keep on the thread-per-read list:
    CoopLds has no 17th column, its store would land in the event buffer;
  - run-length tables of 65 536 entries, which ns_coop_ok must keep there too: coop_error_list's uint16_t would make the step 0."""
import copy

import numpy as np
import pytest

from nanosim_amd import engine as E
from nanosim_amd import model as M
from tests import oracle_lib as O
from tests.test_chain_wave64 import ATrace, insertion_model, zero_match_model
from tests.test_gpu_chain_edges import oracle_pieces
from tests.test_gpu_parity import compare

KNOBS = ("NS_TAIL_BITS", "NS_COOP_MIN", "NS_COOP_SHIFT", "NS_UCOOP_SHIFT", "NS_UCOOP_K")
ALL_ON_THE_WAVE = {"NS_COOP_MIN": "1", "NS_COOP_SHIFT": "0"}
SEED = 20261025


def bins_model(small_model, nbins):
    """nbins match-length columns, previous matches of b bases ask column b (the last: everything from nbins - 1); every column gives
    1 .. 20 bases, a third of the draws the first few (which few depends on the column, so that a wrong column shows)"""
    m = copy.deepcopy(small_model)
    edges = list(range(nbins)) + [1 << 20]
    m.match_markov = [M.EcdfColumn(lo=edges[b], hi_bin=edges[b + 1], hi=np.array([0.3, 1.0]), vhi=np.array([3.0 + b % 3, 21.0]), vlo0=1.0)
                      for b in range(nbins)]
    return m


def long_table_model(small_model, n=65536):
    """the small model with insertion tables of n entries: the small model's own, then entries of 1 - 2^-9 — one insertion in 512 is above
    every entry and gets the table's length"""
    m = copy.deepcopy(small_model)
    m.mix_cdf = [list(c) for c in m.mix_cdf]
    m.mix_cdf[1] = [np.concatenate([np.minimum(np.asarray(c, dtype=np.float64), 1.0 - 2.0 ** -9), np.full(n - len(c), 1.0 - 2.0 ** -9)]) for c in m.mix_cdf[1]]
    return m


def make_cases(small_model, small_ref):
    out = {}
    for name, mdl, kw in (("zero_match", zero_match_model(small_model), dict(n_reads=32, emit_errlog=True)),
                          ("merged_insertions", insertion_model(small_model, 1365), dict(n_reads=16, kind=E.NS_KIND_UNALIGNED, max_len=10 ** 7)),
                          ("bins16", bins_model(small_model, 16), dict(n_reads=48)),
                          ("bins17", bins_model(small_model, 17), dict(n_reads=48)),
                          ("run_65536", long_table_model(small_model), dict(n_reads=64))):
        p = E.make_params(**{**dict(seed=SEED, first_read=0, max_len=small_ref.max_chrom), **kw})
        sizes = dict(bytes_per_read=400000, events_per_read=8000) if name == "merged_insertions" else O.sizes_for_model(mdl, p)
        out[name] = (mdl, p, O.generate(mdl, small_ref, p, **sizes))
    return out


@pytest.fixture(scope="module")
def cases(small_model, small_ref):
    """per case: the model, the parameters and the oracle's batch — computed once, shared by the tests"""
    return make_cases(small_model, small_ref)


def test_the_batches_contain_what_they_are_for(cases, small_model, small_ref, tmp_path):
    from tests.test_chain_wave64 import build, coop_ok
    import ctypes as C
    host = build(str(tmp_path))
    mdl, p, exp = cases["zero_match"]
    t = mdl.to_c()
    found = set()
    for read, seg, gap, m_ref, ev in oracle_pieces(exp, 0):
        tr = ATrace(mdl, t, SEED, read, seg, 0, 2 * len(ev) + 80)
        assert tr.result(m_ref)["n_ev"] == len(ev)                  # (the trace follows the oracle's piece)
        found |= tr.classes(m_ref)
    assert {"collision_at_0_of_a_later_block", "collision_at_a_later_index", "no_two_0_matches_at_0", "no_two_0_matches_at_63"} <= found, found
    mdl, p, exp = cases["merged_insertions"]
    assert int(exp["reads"]["attempts"].sum()) > 20 and int(exp["pieces"]["ref_len"][:16].min()) >= 50      # (no length limit in reach: every redraw is for `range`)
    for name, ok in (("bins16", True), ("bins17", False), ("run_65536", False)):
        mdl, p, exp = cases[name]
        t = mdl.to_c()
        assert coop_ok(mdl) == ok and host.chost_coop_ok(C.byref(t)) == int(ok), name
    for name, last in (("bins16", 15), ("bins17", 16)):
        mdl, p, exp = cases[name]
        asked = 0
        for read, seg, gap, m_ref, ev in oracle_pieces(exp, 0):
            pos = ev["pos"].astype(np.int64)
            adv = np.where(M.ev_type(ev["info"]) != 1, M.ev_len(ev["info"]), 0)
            asked += int((pos[1:] - pos[:-1] - adv[:-1] >= last).sum())          # matches of `last` bases or more: the next iteration asks the last column
        assert asked > 50, (name, asked)
    assert redrawn_for_a_long_run(cases, small_model, small_ref) >= 3


def redrawn_for_a_long_run(cases, small_model, small_ref):
    """the reads of the run_65536 batch that the oracle makes at a later attempt than on the small model's own tables: the two models
    differ only where an insertion draw lies above 1 - 2^-9, which gives 65 536 bases — no event holds them, the read is drawn again"""
    mdl, p, exp = cases["run_65536"]
    plain = O.generate(small_model, small_ref, p, **O.sizes_for_model(small_model, p))
    return int((exp["reads"]["attempts"] > plain["reads"]["attempts"]).sum())


def run(case, small_ref, monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    mdl, p, exp = case
    e = E.Engine(0)
    try:
        e.set_reference(small_ref)
        e.load_model(mdl)
        b = e.generate(p)
        compare(b, exp, p)
        return int(b.info.n_range_redraws)
    finally:
        e.close()


@pytest.mark.gpu
def test_collisions_at_the_first_iteration_of_a_block(cases, small_ref, monkeypatch):
    run(cases["zero_match"], small_ref, monkeypatch, ALL_ON_THE_WAVE)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [None, "1"])
def test_merged_insertions_are_redrawn_as_the_oracle_redraws_them(cases, small_ref, monkeypatch, k):
    n = run(cases["merged_insertions"], small_ref, monkeypatch, {"NS_COOP_MIN": "1", **({"NS_UCOOP_K": k} if k else {})})
    assert 0 < n == int(cases["merged_insertions"][2]["reads"]["attempts"].sum())


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["bins16", "bins17"])
def test_sixteen_and_seventeen_columns_equal_the_oracle_with_every_read_asked_onto_the_wave(cases, small_ref, monkeypatch, name):
    """the batch against the oracle.  Which list a read took is not reported by the engine: that ns_coop_ok refuses the 17 columns is
    asserted on the CPU (first test); here a model it wrongly admitted would store its 17th column into coop_error_list's event buffer"""
    run(cases[name], small_ref, monkeypatch, ALL_ON_THE_WAVE)


@pytest.mark.gpu
def test_a_run_length_table_of_65536_entries_equals_the_oracle_with_every_read_asked_onto_the_wave(cases, small_model, small_ref, monkeypatch):
    """as above: the gate's rule is asserted on the CPU; a model it wrongly admitted would file steps of 0 where the oracle redraws"""
    n = run(cases["run_65536"], small_ref, monkeypatch, ALL_ON_THE_WAVE)
    assert n >= redrawn_for_a_long_run(cases, small_model, small_ref) >= 3
