"""GPU side of tests/test_chain_edges.py: batches whose model has its table edges ON the draws of the batch's own reads (edges_on_draws:
pieces 0 and 128 — the first aligned segment, the first gap or the unaligned read — at attempt 0), through the engine, against the oracle.
Two sizes: 16 reads x 8 iterations, whose image fits LDS whole (tail_bits == 0), and 128 reads x 12 iterations, which gets hot prefixes.
Each runs with every read on the thread-per-read list, with the longest quarter and with all of them on the wave-per-read list
(coop_error_list and its 65 536-cell guide), with NS_TAIL_BITS=3, aligned with the error profile and chimeric with qualities, and as an
unaligned batch on coopk_unaligned_error_list, split with chain_unaligned_error_list, and (all but one read) on the latter alone.
The hits are counted from the oracle's output and the draws (count_hits): a batch that no longer reaches its prepared draws fails — in the
first test, which needs no GPU and runs with the CPU suite.  The last test runs unaligned reads whose first type draw EQUALS one of the
constant rate thresholds of the unaligned lists (RATE_DRAWS of tests/test_chain_edges.py) on the wave-per-read and thread-per-read lists."""
import numpy as np
import pytest

from nanosim_amd import engine as E
from tests import oracle_lib as O
from tests.test_chain_edges import RATE_DRAWS, ST_UEVENT, assert_hits, count_hits, edges_on_draws, philox
from tests.test_gpu_parity import compare
from tests.test_lookup_probe import Packed, build_probe, thr_lt

SEED = 20260926
# first_read and K_match: chosen on the CPU so that the oracle's batches use a prepared draw of every class (check_hits) and the images have
# the sizes the two cases are for (a narrow segment costs its step list: 128 x 12 match edges would not fit LDS at all)
SIZES = dict(small=dict(first_read=2560, n_reads=16, K=8, n_run=64, K_match=8), big=dict(first_read=0, n_reads=128, K=12, n_run=300, K_match=2))
VARIANTS = {"one": dict(last_edge="one"), "below_tiny": dict(last_edge="below", tiny=True)}
KNOBS = ("NS_TAIL_BITS", "NS_COOP_MIN", "NS_COOP_SHIFT", "NS_UCOOP_SHIFT")
ALIGNED_ENVS = dict(thread_per_read={"NS_COOP_MIN": "1000000000"}, wave_per_read={"NS_COOP_MIN": "1", "NS_COOP_SHIFT": "2"},
                    wave_per_read_all={"NS_COOP_MIN": "1", "NS_COOP_SHIFT": "0"}, tail3={"NS_TAIL_BITS": "3"})
UNALIGNED_ENVS = dict(ucoop_shift0={"NS_UCOOP_SHIFT": "0"}, ucoop_shift1={"NS_COOP_MIN": "1", "NS_UCOOP_SHIFT": "1"},
                      thread_per_read={"NS_COOP_MIN": "1", "NS_UCOOP_SHIFT": "31"})
BATCHES = dict(aligned_errlog=dict(emit_errlog=True), chimeric_fastq=dict(chimeric=True, fastq=True), unaligned=dict(kind=E.NS_KIND_UNALIGNED))


def oracle_pieces(exp, first_read, attempt=0):
    """(read, seg, unaligned?, m_ref, events) of every piece of the oracle's batch that was made at `attempt` (a read that was drawn again
    has other draws); pieces alternate segment, gap, segment ...: ids pi >> 1 and 128 + (pi >> 1).  m_ref: the final middle_ref, which is
    positive exactly when m_ref was"""
    out = []
    for i, rd in enumerate(exp["reads"]):
        if int(rd["attempts"]) != attempt:
            continue
        for pi in range(int(rd["n_pieces"])):
            pc = exp["pieces"][int(rd["piece_off"]) + pi]
            gap = bool(pc["kind"])
            out.append((first_read + i, (128 if gap else 0) + (pi >> 1), gap, int(pc["ref_len"]), exp["events"][int(pc["ev_off"]):int(pc["ev_off"]) + int(pc["n_ev"])]))
    return out


def make_case(small_model, small_ref, size, variant):
    s = SIZES[size]
    Ed = edges_on_draws(small_model, SEED, range(s["first_read"], s["first_read"] + s["n_reads"]), (0, 128), 0, s["K"], n_run=s["n_run"], K_match=s["K_match"], aligned_segs=(0,), **VARIANTS[variant])
    out = dict(edged=Ed, batches={})
    for name, kw in BATCHES.items():
        p = E.make_params(seed=SEED, first_read=s["first_read"], n_reads=s["n_reads"], max_len=small_ref.max_chrom, **kw)
        exp = O.generate(Ed.model, small_ref, p, **O.sizes_for_model(Ed.model, p))
        pieces = [x for x in oracle_pieces(exp, s["first_read"]) if (x[0], x[1]) in Ed.ev]
        out["batches"][name] = (p, exp, count_hits(Ed, pieces))
    return out


@pytest.fixture(scope="module")
def cases(small_model, small_ref):
    """per (size, variant): the model and, per batch, its parameters, the oracle's output and the hits — computed once, shared by the environments"""
    return {(size, variant): make_case(small_model, small_ref, size, variant) for size in SIZES for variant in VARIANTS}


def check_hits(case):
    for name, (_, _, hits) in case["batches"].items():
        assert_hits(hits, ("unaligned",) if name == "unaligned" else ("aligned",))


def test_the_batches_reach_their_prepared_draws_and_have_the_images_they_are_for(cases, tmp_path):
    L = build_probe(str(tmp_path), gpu=False)
    for (size, variant), case in cases.items():
        check_hits(case)
        P = Packed(L, case["edged"].model)
        try:
            assert P.whole
            if size == "small":
                assert P.ct.tail_bits == 0 and 8 * P.ct.n_words_lds <= 24 * 1024       # the image fits LDS whole
            else:
                assert P.ct.tail_bits > 0 and 8 * P.ct.n_words_lds <= 44 * 1024        # hot prefixes in LDS, the full columns behind them
        finally:
            P.close()


def _run(case, small_ref, monkeypatch, env, names):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    e = E.Engine(0)
    try:
        e.set_reference(small_ref)
        e.load_model(case["edged"].model)
        for name in names:
            p, exp, _ = case["batches"][name]
            compare(e.generate(p), exp, p)
    finally:
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("env", list(ALIGNED_ENVS))
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("size", list(SIZES))
def test_aligned_and_chimeric_batches_equal_the_oracle(cases, small_ref, monkeypatch, size, variant, env):
    case = cases[(size, variant)]
    check_hits(case)
    _run(case, small_ref, monkeypatch, ALIGNED_ENVS[env], ("aligned_errlog", "chimeric_fastq"))


@pytest.mark.gpu
@pytest.mark.parametrize("env", list(UNALIGNED_ENVS))
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("size", list(SIZES))
def test_unaligned_batches_equal_the_oracle(cases, small_ref, monkeypatch, size, variant, env):
    case = cases[(size, variant)]
    check_hits(case)
    _run(case, small_ref, monkeypatch, UNALIGNED_ENVS[env], ("unaligned",))


@pytest.mark.gpu
@pytest.mark.parametrize("env", list(UNALIGNED_ENVS))
def test_unaligned_reads_whose_type_draw_equals_a_rate_threshold(small_model, small_ref, monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in UNALIGNED_ENVS[env].items():
        monkeypatch.setenv(k, v)
    e = E.Engine(0)
    try:
        e.set_reference(small_ref)
        e.load_model(small_model)
        for seed, read, rate in RATE_DRAWS:
            assert philox(seed, read, ST_UEVENT, 128, 0, 0)[0] == int(thr_lt(rate))
            p = E.make_params(seed=seed, first_read=read - 1, n_reads=3, max_len=small_ref.max_chrom, kind=E.NS_KIND_UNALIGNED)
            exp = O.generate(small_model, small_ref, p)
            assert int(exp["reads"]["attempts"][1]) == 0 and int(exp["pieces"]["ref_len"][1]) > 0      # the read is made at the attempt of that draw
            compare(e.generate(p), exp, p)
    finally:
        e.close()
