"""GPU parity of the training side's intron-retention model ("Intron retention: the Markov counts"): ns_ir_train (k_ir_walk,
csrc/ns_train.h) against what the REAL src/model_intron_retention.py counted and wrote (tests/golden/reference_ir_train.json.gz) and
against the same walk compiled for the host — on the whole fixture, on its first 1, 63, 65 and 257 reads, in another order of the
reads, after larger and smaller calls on the same engine, next to a read of 5 000 CIGAR ops, and between other training calls."""
import numpy as np
import pytest

from nanosim_amd import characterize
from nanosim_amd import engine as EN
from tests import test_read_lengths
from tests.test_ir_train import (BAD_CIGARS, HAND, NONE, build_host_walk, call, check_bad, check_bad_corners, check_files, check_fixture, check_hand, check_union,
                                 check_validation, hand_tables, load_fixture, write_inputs)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    return load_fixture()


@pytest.fixture(scope="module")
def host():
    return build_host_walk()


@pytest.fixture(scope="module")
def eng():
    e = EN.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def packed(fx, tmp_path_factory):
    """(tables, the fixture's reads as (cigar, start, chrom id, trx id)), taken from the files once"""
    gff, g_sam, t_sam = write_inputs(fx, tmp_path_factory.mktemp("ir"))
    tables = characterize.ir_tables(characterize.ir_introns(gff))
    reads = [(r.cigar, r.start, tables["chrom_id"].get(characterize._strip_chr(r.chrom), NONE), tables["trx_id"].get(r.trx, NONE))
             for r in characterize.ir_alignments(g_sam, t_sam)]
    assert len(reads) == 290
    return tables, reads


def equal_to_host(eng, host, reads, tables):
    g, h = call(eng, reads, tables), call(host, reads, tables)
    assert g == h
    return g


def test_gpu_fixture_per_read_and_in_total(fx, eng, tmp_path):
    """290 reads: two workgroups, the sorted visiting order; then every read alone: index order"""
    got = check_fixture(eng, fx, tmp_path)[2]
    assert got["ms_kernel"] > 0
    print("ms_kernel %.3f" % got["ms_kernel"])


@pytest.mark.parametrize("case", ["start_row_0", "no_ir_row_0", "ir_row_0", "both_state_rows_0"])
def test_gpu_files_equal_the_reference(fx, eng, tmp_path, case):
    check_files(eng, fx, tmp_path, case)


def test_gpu_read_counts_orders_and_repeats(fx, eng, host, packed):
    tables, reads = packed
    want = equal_to_host(eng, host, reads, tables)
    assert want[0] == fx["first"] + fx["states"] and want[3:] == (0, len(reads))
    per = {p["qname"]: p["counts"] for p in fx["per_read"]}
    counts_of = lambda n: [sum(per[q][i] for q in fx["order"][:n]) for i in range(6)]
    # 1 read, one short of a wavefront (index order), one more than a wavefront (sorted), one more than a workgroup; then the full call
    # again behind the smaller ones and the smaller behind the full one: nothing of a call stays on the engine
    for n in (1, 63, 65, 257, len(reads), 63, 257):
        g = equal_to_host(eng, host, reads[:n], tables)
        assert g[0] == counts_of(n) and g[1] == want[1][:n] and g[3:] == (0, n)
    assert call(eng, reads, tables) == want
    # another order of the reads: the same totals and bitmap, the states permuted with them
    perm = np.random.default_rng(3).permutation(len(reads)).tolist()
    g = call(eng, [reads[i] for i in perm], tables)
    assert g[0] == want[0] and g[2] == want[2] and g[1] == [want[1][i] for i in perm]
    # the same reads many times over: 32 workgroups add to the same six counters and OR the same words
    many = call(eng, reads * 28, tables)
    assert many[0] == [28 * v for v in want[0]] and many[2] == want[2] and many[1] == want[1] * 28


def test_gpu_no_read(eng, host):
    assert call(eng, []) == call(host, []) == ([0] * 6, [], [], 0, 0)


def test_gpu_a_long_cigar_next_to_one_op_reads(eng, host):
    """one read of 5 001 ops that walks through the 33 introns of the second transcript again and again next to 300 reads of one op: the
    longest walk is visited first, its wavefront waits for it alone"""
    ops = "".join("%dM%d%s" % (30 + i % 9, 1 + i % 4, "DNI"[i % 3]) for i in range(2500)) + "7M"
    assert sum(1 for c in ops if not c.isdigit()) == 5001
    tables = hand_tables()
    reads = [("%dM" % (40 + i % 90), 950 + 13 * i, 1, 1) for i in range(150)] + [(ops, 900, 1, 1)] + [("%d=" % (60 + i % 50), 90 + i, 0, i % 2) for i in range(150)]
    g = equal_to_host(eng, host, reads, tables)
    assert g[3:] == (0, 301) and g[1][150] in (1, 2) and 2 in g[1] and 1 in g[1]
    assert call(eng, [reads[150]], tables) == call(host, [reads[150]], tables)
    bad = list(reads)
    bad[150] = (ops + "5", 900, 1, 1)                          # the long one ends in a count without an op
    g = equal_to_host(eng, host, bad, tables)
    assert g[3:] == (1, 150) and g[1][150] == 0


def test_gpu_hand_made_reads(eng, host):
    for case in HAND:
        check_hand(eng, case)
    check_union(eng)
    equal_to_host(eng, host, [c[1] for c in HAND] * 20, hand_tables())


def test_gpu_bad_cigars(eng, host):
    for bad in BAD_CIGARS:
        check_bad(eng, bad)
    check_bad_corners(eng)
    reads = [("200M", 50, 0, 0)] * 300 + [("50M7", 50, 0, 0)] + [("%dS200M" % i, 50, 0, 0) for i in range(10)] + [("Z", 50, 0, NONE)]
    g = equal_to_host(eng, host, reads, hand_tables())
    assert g[3:] == (2, 300) and g[0] == [0, 310, 0, 0, 310, 0]


def test_gpu_argument_checks(eng):
    check_validation(eng, EN.EngineError)
    with pytest.raises(EN.EngineError, match="ns_ir_train"):
        call(eng, [("200M", 50, 7, 0)])
    assert call(eng, [("200M", 50, 0, 0)])[0] == [0, 1, 0, 0, 1, 0]          # the engine goes on after a refused call


def test_gpu_interleaved_with_another_training_call(fx, eng, host, packed):
    """ns_ir_train between ns_read_lengths calls on one engine (the length sort of both takes its temporary storage from the context):
    every result equals the host walk's, that of an engine that has done nothing else, and — the lengths — the reference's"""
    tables, reads = packed
    lfx = test_read_lengths.load_fixture()
    want_ir = call(host, reads, tables)
    test_read_lengths.check_genome(eng, lfx)
    assert call(eng, reads, tables) == want_ir
    assert call(eng, reads[:64], tables) == call(host, reads[:64], tables)
    test_read_lengths.check_genome(eng, lfx)
    assert call(eng, reads[:65], tables) == call(host, reads[:65], tables)
    test_read_lengths.check_transcriptome(eng, lfx)
    assert call(eng, reads, tables) == want_ir
    fresh = EN.Engine(0)
    try:
        assert call(fresh, reads, tables) == want_ir
    finally:
        fresh.close()
