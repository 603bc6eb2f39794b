"""GPU side of tests/test_chain_guide.py: with the octave guide of the ECDF columns (guide_cell, ns_device.h) the records and events of
2 000 aligned reads equal the oracle's (which has no guide) on the models that send the match look-up of k_chain down each of its paths —
once with every read on the thread-per-read list (NS_COOP_MIN out of reach) and once with the longest quarter on the wave-per-read list
(NS_COOP_MIN=1), which passes the same guide to ecdf_lookup_gv / ecdf_lookup_g."""
import numpy as np
import pytest

from nanosim_amd import engine as E
from nanosim_amd import model as M
from nanosim_amd import synth
from tests import oracle_lib as O
from tests.test_chain_guide import BENCH_SEED, _specs, build_host
from tests.test_gpu_parity import compare

pytestmark = pytest.mark.gpu

# model -> (spec name or None for the small model, environment of the engine)
MODELS = dict(small=(None, {}),
              big=("big", {"NS_TAIL_BITS": "8"}),        # prefixes that one draw in 256 leaves: the full columns in global memory under load
              long=("long", {}),                         # image in global memory, previous matches >= 256
              octaves=("octaves", {}))                   # 400-row ECDFs of 10^6 training alignments: segments in every octave of the guide, dozens
                                                         # in its last cell (and prefixes in LDS that end where that cell starts)
LISTS = dict(thread_per_read={"NS_COOP_MIN": "1000000000"}, wave_per_read={"NS_COOP_MIN": "1", "NS_COOP_SHIFT": "2"})


@pytest.fixture(scope="module")
def cases(tmp_path_factory, small_model, small_ref):
    """per model: the model, the parameters of the batch and what the oracle makes of them — computed once, shared by both lists"""
    tmp = tmp_path_factory.mktemp("gpu_chain_guide")
    out = {}
    for name, (spec, _) in MODELS.items():
        if spec is None:
            mdl = small_model
        else:
            prefix = str(tmp / name / "training")
            synth.write_model(prefix, synth.SynthModelSpec(n_train=1_000_000, seed=BENCH_SEED, ecdf_rows=400) if spec == "octaves" else _specs()[spec],
                              write_pkl=False)
            mdl = M.load_model(prefix)
        p = E.make_params(seed=BENCH_SEED, first_read=3, n_reads=2000, max_len=small_ref.max_chrom, emit_errlog=True)
        out[name] = (mdl, p, O.generate(mdl, small_ref, p))
    return out


def test_the_octaves_model_has_segments_in_every_octave_and_in_the_last_cell(cases, tmp_path):
    """what the `octaves` case is for: every match-length column of its model has an ECDF edge inside every octave of the guide and inside
    the guide's last cell, and the batch draws from that cell"""
    L = build_host(str(tmp_path))
    octaves, cells = L.cg_octaves(), L.cg_cells()
    start_p = np.array([L.cg_cell_start(c) for c in range(cells)] + [1 << 32], dtype=np.float64) * 2.0 ** -32
    mdl = cases["octaves"][0]
    for c in mdl.match_markov:
        hi = np.asarray(c.hi, dtype=np.float64)
        hi = hi[hi < 1.0]
        for l in range(octaves):
            assert ((hi >= start_p[32 * l]) & (hi < start_p[32 * (l + 1)])).any(), l
        assert (hi >= start_p[cells - 1]).sum() >= 3          # ... the last cell holds three or more: its draws need the bisection
    n_events = len(cases["octaves"][2]["events"])
    assert n_events * (1.0 - start_p[cells - 1]) > 5          # expected draws of the batch inside the last cell


@pytest.mark.parametrize("which", list(LISTS))
@pytest.mark.parametrize("name", list(MODELS))
def test_records_and_events_equal_the_oracle(cases, small_ref, monkeypatch, name, which):
    mdl, p, exp = cases[name]
    for k in ("NS_TAIL_BITS", "NS_COOP_MIN", "NS_COOP_SHIFT"):
        monkeypatch.delenv(k, raising=False)
    for k, v in {**MODELS[name][1], **LISTS[which]}.items():
        monkeypatch.setenv(k, v)
    e = E.Engine(0)
    try:
        e.set_reference(small_ref)
        e.load_model(mdl)
        compare(e.generate(p), exp, p)
    finally:
        e.close()
