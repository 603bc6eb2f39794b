"""The cases of tests/test_gpu_record_strands.py and what they must contain, on the oracle alone.  The tile loop of the record kernels
(materialise_piece, nanosim_amd/csrc/ns_materialise.h) exists once per strand, the destination of a piece is folded into one base address
per piece (PieceOut), and what only a queued tile reads is fetched where it is needed: the cases below put forward AND reversed reads on
every alignment of the sequence line, on pieces whose first and last chunks are partial, full, or cut by a tile end, on tiles that end
early, and on tiles that go to the slow queue.  Which of these a batch holds is counted here with the replay of tests/kernel_classes.py
(never with a data path); a class that no read of its case reaches fails the test, so the GPU comparison cannot pass by missing them."""
import collections

import pytest

from nanosim_amd import engine as E
from tests import kernel_classes as K
from tests import oracle_lib as O
from tests.test_record_rare_paths import SEED, build_models, build_refs

STRANDS = ("fwd", "rev")
LENGTHS = (1, 15, 16, 17, 31, 33, 2047, 2048, 2049)
SHORT = [l for l in LENGTHS if l < 2000]
LONG = [l for l in LENGTHS if l > 2000]


def both(names):
    return ["%s:%s" % (s, n) for s in STRANDS for n in names]


PHI = both(["phi_%d" % i for i in range(16)])
HEADS = ["head_%d" % i for i in range(17)]
PARTIAL = both(["first_chunk_partial", "first_chunk_full", "last_chunk_partial", "last_chunk_full"])
EARLY = both(["tile_cnt_62", "tile_cnt_63", "tile_64_events_cut_on_chunk_boundary", "tile_ends_early"])
# (id, reference, model, parameters, classes of strand_classes() the case must reach)
CASES = [
    # reads of a few bases to a few chunks: every alignment, every short length, pieces inside one chunk
    ("tiny-fasta", "iupac", "letters", dict(n_reads=1000, median_len=16, sd_len=0.9, min_len=1), PHI + PARTIAL + both(["len_%d" % l for l in SHORT])),
    ("tiny-fastq-uracil", "iupac", "letters", dict(n_reads=1000, median_len=16, sd_len=0.9, min_len=1, fastq=True, uracil=True),
     PHI + PARTIAL + both(["len_%d" % l for l in SHORT])),
    # a tile is 2048 output bytes: pieces that end one byte short of it, on it, one byte into the next (the events move a piece's length
    # by +- 80 bytes around 1.04 x the drawn one: 3 000 reads put a handful on every exact length and strand)
    ("tile-fasta-uracil", "iupac", "letters", dict(n_reads=3000, median_len=1970, sd_len=0.003, min_len=1, uracil=True),
     both(["len_%d" % l for l in LONG]) + both(["piece_second_tile"])),
    ("tile-fastq", "iupac", "letters", dict(n_reads=3000, median_len=1970, sd_len=0.003, min_len=1, fastq=True),
     both(["len_%d" % l for l in LONG]) + both(["piece_second_tile"])),
    # more events than a tile stages: the tile ends early, on a chunk boundary
    ("dense-fasta", "iupac", "dense", dict(n_reads=150), EARLY),
    ("dense-fastq", "iupac", "dense", dict(n_reads=150, fastq=True), EARLY),
    # several pieces per read: every piece but the first starts wherever the one before it ended
    ("chimeric-fasta", "iupac", "chim", dict(n_reads=200, chimeric=True), both(["piece_not_first", "piece_gap"]) + PHI),
    ("chimeric-fastq-uracil", "odd", "chim", dict(n_reads=200, chimeric=True, fastq=True, uracil=True), both(["piece_not_first", "piece_gap"])),
    # the two passes of -k 5 (the census covers the first pass without -k: strands and heads only)
    ("kmer-bias-5-fasta", "iupac", "letters", dict(n_reads=200, kmer_bias=5), both(["read"]) + HEADS),
    ("kmer-bias-5-fastq-uracil", "iupac", "letters", dict(n_reads=200, kmer_bias=5, fastq=True, uracil=True), both(["read"])),
    ("kmer-bias-5-tiny", "iupac", "letters", dict(n_reads=300, kmer_bias=5, fastq=True, median_len=40, sd_len=0.9, min_len=1), both(["read"])),
    # the rare paths: tiles that straddle the origin of a circular reference go to the slow queue, tiles beyond it move their base
    ("circular-fasta", "circ", "letters", dict(n_reads=200), both(["tile_slow_queue", "tile_beyond_origin", "piece_wraps_origin"])),
    ("circular-fastq", "circ", "letters", dict(n_reads=200, fastq=True, emit_errlog=True), both(["tile_slow_queue", "tile_beyond_origin"])),
    ("circular-kmer-bias-5", "circ", "letters", dict(n_reads=200, kmer_bias=5, fastq=True), both(["read"])),
]


def strand_classes(batch, ref, prm):
    """classes of the reads and pieces of an aligned batch by strand: "<fwd|rev>:<class>" (and head_<n> for head lengths 0 .. 16)"""
    C = collections.Counter()
    for r in batch["reads"]:
        if not int(r["flags"]):
            C[("rev" if int(r["reversed"]) else "fwd") + ":read"] += 1
            if int(r["head"]) <= 16:
                C["head_%d" % int(r["head"])] += 1
    if int(prm.kmer_bias):
        return dict(C)
    for r, seq, p, pq, phi in K.record_pieces(batch, prm):
        s = "rev" if int(r["reversed"]) else "fwd"
        out_len = int(p["out_len"])
        C[s + ":phi_%d" % phi] += 1                                          # the piece's chunk grid in the destination (PieceOut::phi)
        if out_len in LENGTHS:
            C[s + ":len_%d" % out_len] += 1
        if out_len:
            C[s + (":first_chunk_partial" if phi else ":first_chunk_full")] += 1     # chunk 0 starts in front of the piece: shifted down, count < 16
            C[s + (":last_chunk_partial" if (out_len - phi) & 15 else ":last_chunk_full")] += 1
        C[s + ":piece_not_first"] += pq != int(r["head"])
        C[s + ":piece_gap"] += int(p["kind"]) != 0
        os_, pl, ty, ln, epos, rp = K._events(batch, p)
        span = K._Span(ref, p)
        C[s + ":piece_wraps_origin"] += span.wraps
        for t in K.piece_tiles(os_, pl, ty, rp, out_len, phi, span):
            C[s + ":piece_second_tile"] += t["M0"] > 0
            C[s + ":tile_ends_early"] += t["cut"] is not None
            C[s + ":tile_64_events_cut_on_chunk_boundary"] += t["cut"] == "chunk"
            C[s + ":tile_slow_queue"] += t["queued"] is not None
            if t["queued"] is None:
                C[s + ":tile_cnt_%d" % t["cnt"]] += 1
                C[s + ":tile_beyond_origin"] += t.get("origin") == "beyond"
    return dict(C)


_ORACLE = {}


def oracle_case(cid, rname, mname, case, models, refs):
    """(params, oracle batch) of one case, computed once for the reach check and the GPU comparison"""
    if cid not in _ORACLE:
        kw = dict(seed=SEED, first_read=0, max_len=int(refs[rname].max_chrom))
        kw.update(case)
        p = E.make_params(**kw)
        _ORACLE[cid] = (p, O.generate(models[mname], refs[rname], p, bytes_per_read=80000, events_per_read=8000))
    return _ORACLE[cid]


def check_reach(cid, rname, p, exp, reach, refs):
    assert len(exp["reads"]) == p.n_reads
    cen = strand_classes(exp, refs[rname], p)
    empty = [name for name in reach if not cen.get(name, 0)]
    assert not empty, "case %s reaches none of %s" % (cid, empty)
    return cen


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    return build_models(tmp_path_factory.mktemp("record_strands"))


@pytest.fixture(scope="module")
def refs():
    return build_refs()


@pytest.mark.parametrize("cid,rname,mname,case,reach", CASES, ids=[c[0] for c in CASES])
def test_cases_reach_their_classes(models, refs, cid, rname, mname, case, reach):
    """on the oracle alone: every case holds the inputs it exists for"""
    p, exp = oracle_case(cid, rname, mname, case, models, refs)
    check_reach(cid, rname, p, exp, reach, refs)


def test_the_three_classes_of_the_strand_loops_are_not_empty(models, refs):
    """summed over the cases: reversed reads with a partial first chunk, tiles that end early, tiles that go to the slow queue — and the same
    on the forward strand"""
    tot = collections.Counter()
    for cid, rname, mname, case, reach in CASES:
        p, exp = oracle_case(cid, rname, mname, case, models, refs)
        tot.update(strand_classes(exp, refs[rname], p))
    for name in both(["first_chunk_partial", "tile_ends_early", "tile_slow_queue"]):
        assert tot[name] > 0, name
    for h in range(17):
        assert tot["head_%d" % h] > 0, "no read with a head of %d bases" % h
