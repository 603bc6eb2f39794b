"""The training-side calls and the simulation on ONE context, interleaved.  The length sort of the counting calls (order_by_length) takes
its temporary storage from the context's scan_tmp, which the scans and sorts of ns_generate use as well; everything else a counting call
allocates is its own and gone when it returns (CallScratch, csrc/ns_train_calls.h).  So: generate, count, generate, count ... on one engine,
with 65 alignments (the fewest that are sorted) and with 64 (the most that are visited in index order), and every result compared with
the walk compiled for the host, with an engine that has done nothing else, and — the reads — with the oracle.  No new kernel runs here
(k_* of csrc/ns_train.h are covered by tests/test_gpu_zz*), hence no child run."""
import numpy as np
import pytest

from nanosim_amd import characterize
from nanosim_amd import engine as E
from tests import oracle_lib as O
from tests import test_basequal, test_hp_train
from tests.test_characterize import fx, fx_maf, host_walk, same_counts  # noqa: F401  (fx, fx_maf, host_walk: its fixtures, under their own names)

pytestmark = pytest.mark.gpu
N_SORTED, N_INDEX = 65, 64
SEED = 20260926                     # (the parameters of smoke())


@pytest.fixture(scope="module")
def inputs(fx, fx_maf):
    """the first 65 alignments of the four fixtures"""
    d = dict(cs=fx["cs"][:N_SORTED], maf=[tuple(p) for p in fx_maf["maf"][:N_SORTED]],
             qual=test_basequal.load_fixture()["alignments"][:N_SORTED], hp=test_hp_train.load_fixture()["records"][:N_SORTED])
    assert all(len(v) == N_SORTED for v in d.values())
    return d


@pytest.fixture(scope="module")
def host_results(inputs, host_walk):
    """{(call, n): the host-compiled walk's result on the first n inputs}, computed once"""
    hq, hh = test_basequal.build_host_walk(), test_hp_train.build_host_walk()
    out = {}
    for n in (N_SORTED, N_INDEX):
        out["cs", n] = host_walk(inputs["cs"][:n])
        out["maf", n] = host_walk(inputs["maf"][:n], maf=True)
        out["qual", n] = characterize.count_qualities(hq, inputs["qual"][:n])
        out["hp", n] = characterize.count_homopolymers(hh, inputs["hp"][:n], records=True)
    return out


def count_on(eng, call, data):
    if call == "cs":
        return characterize.count(eng, data)
    if call == "maf":
        return characterize.count_maf(eng, data)
    if call == "qual":
        return characterize.count_qualities(eng, data)
    return characterize.count_homopolymers(eng, data, records=True)


def assert_same(call, got, want):
    """every entry but the kernel time; the cs / MAF tables through same_counts (the two match matrices may differ in size)"""
    if call in ("cs", "maf"):
        same_counts(got, want)
        return
    assert sorted(k for k in got if k != "ms_kernel") == sorted(k for k in want if k != "ms_kernel")
    for k, v in want.items():
        if k != "ms_kernel":
            assert np.array_equal(got[k], v), (call, k)


def test_counting_calls_between_generate_calls_on_one_context(small_model, small_ref, inputs, host_results):
    p = E.make_params(seed=SEED, first_read=0, n_reads=256, kind=E.NS_KIND_ALIGNED, fastq=True, chimeric=True, max_len=small_ref.max_chrom,
                      emit_errlog=True)
    exp = O.generate(small_model, small_ref, p)
    eng = E.Engine(0)
    try:
        eng.set_reference(small_ref)
        eng.load_model(small_model)

        def generate():
            b = eng.generate(p)
            return b.records().tobytes(), b.errlog().tobytes()

        def count(call, n):
            data = inputs[call][:n]
            got = count_on(eng, call, data)
            assert_same(call, got, host_results[call, n])
            if call == "cs":
                assert host_results[call, n]["n_skip"] == 0
            fresh = E.Engine(0)
            try:
                want = count_on(fresh, call, data)
            finally:
                fresh.close()
            assert_same(call, got, want)
            if call in ("cs", "maf"):
                assert got["match_list"].shape == want["match_list"].shape
            assert got["ms_kernel"] > 0

        runs = [generate()]
        count("cs", N_SORTED)
        runs.append(generate())
        count("qual", N_SORTED)
        count("hp", N_SORTED)
        count("maf", N_SORTED)
        for call in ("cs", "qual", "hp", "maf"):
            count(call, N_INDEX)
        runs.append(generate())
    finally:
        eng.close()
    assert runs[0] == runs[1] == runs[2]
    assert runs[0][0] == exp["records"].tobytes() and runs[0][1] == exp["errlog"].tobytes()
    assert len(runs[0][0]) > 0 and len(runs[0][1]) > 0
