"""The record kernels on both strands, byte for byte against the oracle: the tile loop is instantiated per strand, a piece's destination is
one base address (forward: ascending from it, reversed: descending), --uracil is a parameter of the kernel, and what only a queued tile
reads — the slow-tile queue, the read's number, the chromosome's length — is fetched on that path.  Forward and reversed reads on every
alignment of the sequence line, pieces of 1 .. 2049 bytes, tiles of 62 / 63 / more than 63 events, FASTA / FASTQ / both passes of -k 5 /
chimeric batches with --uracil on and off; then the rare paths: pieces across the origin of a circular reference, 64 events at one output
offset, a slow-tile queue that has to grow.  Cases and their reach check (on the oracle alone) are those of tests/test_record_strands.py."""
import copy

import numpy as np
import pytest

from nanosim_amd import engine as E
from nanosim_amd import model as M
from tests import oracle_lib as O
from tests.test_gpu_parity import compare
from tests.test_record_rare_paths import SEED, build_models, build_refs
from tests.test_record_strands import CASES, check_reach, oracle_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    return build_models(tmp_path_factory.mktemp("gpu_record_strands"))


@pytest.fixture(scope="module")
def refs():
    return build_refs()


@pytest.fixture(scope="module")
def engines(refs):
    made = {}

    def get(rname):
        if rname not in made:
            e = E.Engine(0)
            e.set_reference(refs[rname])
            made[rname] = e
        return made[rname]
    yield get
    for e in made.values():
        e.close()


@pytest.mark.parametrize("cid,rname,mname,case,reach", CASES, ids=[c[0] for c in CASES])
def test_gpu_strands_equal_oracle(engines, models, refs, cid, rname, mname, case, reach):
    p, exp = oracle_case(cid, rname, mname, case, models, refs)
    check_reach(cid, rname, p, exp, reach, refs)
    eng = engines(rname)
    eng.load_model(models[mname])
    compare(eng.generate(p), exp, p)


@pytest.mark.parametrize("fastq,uracil", [(False, True), (True, False)])
def test_gpu_64_events_at_one_offset_on_both_strands(models, fastq, uracil):
    """the second pass of -k 5 on a reference of runs of five whose every run is re-sampled to nothing (the construction of
    tests/test_gpu_parity.py::test_dense_homopolymer_edits_take_the_slow_tiles): more deletions at ONE output offset than a tile stages, so
    the tile is queued from inside the tile loop — on forward and on reversed reads"""
    m = copy.deepcopy(models["letters"])
    for base in ("AT", "CG"):
        m.hp[base] = dict(m.hp[base], const=-50.0, alpha1=0.0, betas=[0.0] * len(m.hp[base]["betas"]), intercept=0.1, slope=0.0)
    seq = np.frombuffer((b"AAAAACCCCCGGGGGTTTTT" * 3000), dtype=np.uint8).copy()
    ref = M.Reference(["runs"], seq, np.array([0, len(seq)], dtype=np.uint64), np.array([0], dtype=np.uint8))
    p = E.make_params(seed=SEED, first_read=0, n_reads=120, fastq=fastq, uracil=uracil, kmer_bias=5, min_len=1, max_len=ref.max_chrom)
    exp = O.generate(m, ref, p, bytes_per_read=80000, events_per_read=8000)
    rd, pc = exp["reads"], exp["pieces"]
    lost = pc["ref_len"].astype(np.int64)[rd["piece_off"]] - pc["out_len"][rd["piece_off"]]
    for strand in (0, 1):                       # hundreds of runs deleted in a row, on either strand
        assert int(np.max(lost[(rd["reversed"] != 0) == bool(strand)])) > 64 * 5, strand
    e = E.Engine(0)
    try:
        e.set_reference(ref)
        e.load_model(m)
        compare(e.generate(p), exp, p)
    finally:
        e.close()


def test_gpu_slow_queue_grows_between_batches(models, refs):
    """a fresh engine's first call allocates the slow-tile queue for its batch (launch_materialise: n / 4 + 4096 tiles, plus an eighth and
    4 KB: 4 882 slots for 64 reads); a batch of 3 400 reads needs 4 946 — a NEW buffer, whose counter the launch has to zero — and both
    queue the tiles that straddle the origin of the circular reference"""
    e = E.Engine(0)
    try:
        e.set_reference(refs["circ"])
        e.load_model(models["letters"])
        for n, kw in ((64, dict()), (3400, dict(median_len=1500, sd_len=0.3))):
            p = E.make_params(seed=SEED + n, first_read=0, n_reads=n, max_len=int(refs["circ"].max_chrom), fastq=True, **kw)
            exp = O.generate(models["letters"], refs["circ"], p, bytes_per_read=80000, events_per_read=8000)
            cen = check_reach("queue-%d" % n, "circ", p, exp, ["fwd:tile_slow_queue", "rev:tile_slow_queue"], refs)
            assert cen["fwd:tile_slow_queue"] + cen["rev:tile_slow_queue"] >= 4
            compare(e.generate(p), exp, p)
    finally:
        e.close()
