"""Whole batches at the input classes of the three kernels that write almost every output byte: the tile loop
of k_materialise (materialise_piece), the body of k_materialise_dense (dense_piece) and k_errlog<BUF>.  Which branch they take is a pure
function of the batch, so tests/kernel_classes.py replays their case selection over an oracle batch and counts the classes.

The CPU half (every run): each case reaches the classes it exists for at least REACH_MIN times on the oracle alone
(test_cases_reach_their_classes); the replay is held against the batch itself (tiles partition the pieces, every event is taken once,
the predicted error-profile rows are the rows of the oracle's image: test_replay_self_check); and the aligned chain never puts more
than 32 events into one 16-byte chunk (test_aligned_chain_never_packs_a_chunk).  The gpu half holds the engine against the oracle with
test_gpu_parity.compare.

The census.  "before" = the cases without -k of test_gpu_parity.CASES, test_dense_events_and_long_payloads' model (linear and circular),
the circular-reference cases, test_gpu_metagenome.CASES and one transcriptome batch, run through the oracle; "cases" = the cases of
this file; scripts/kernel_census.py prints both columns.  max_* are maxima, the others sums; of phi_*, mis_*, al_*, letters_8_at_*,
rows_unstaged_nl_* and len_q*_r* the table shows the smallest of the group.
The pieces without events and most tiles with cnt == 0 of "before" are those of --perfect batches, which have no event at all; the
unstaged error-profile blocks of "before" are the metagenome's (species-chromosome names):

    record_classes (materialise_piece)                before     cases
    pieces                                              6966      3058
    piece_gap                                            132       201
    phi_0 .. phi_15 (least)                              410       174
    strand_forward                                      1544      1750
    strand_reverse                                      5422      1308
    piece_shorter_than_16                                 36       320
    piece_no_event                                      1002       280
    event_at_piece_end                                   124        88
    tiles                                              33964     11412
    tile_cnt_0                                          4175       457
    tile_cnt_1_62                                      18954      7526
    tile_cnt_63                                        10537      3413
    tile_nc_above_64                                   21132      7903
    tile_nc_128                                         9235      3605
    tile_first_A0_negative                              6440      2825
    tile_last_chunk_partial                             6465      2830
    tile_cut_on_chunk_boundary                         17669      4787
    tile_cut_inside_chunk                                  0         0   unreachable, see below
    tile_64_events_at_one_offset                           0         0   unreachable, see below
    class_word_carry                                       0         0   unreachable, see below
    tile_mid_piece_chunk0_before_M0                        0         0   unreachable, see below
    tile_L0_start                                      10012      3029
    tile_L0_mis                                        10899      3505
    tile_L0_ins                                         6728      2504
    tile_L0_del                                         6027      2358
    letters_1_7                                       957077    306206
    letters_8_at_0 .. _3 (least)                        2704       553
    letters_9_16                                       34329      6767
    letters_above_16                                   17568      3685
    payload_continued                                   3618      1077
    payload_continued_beyond_tile                          0        85
    payload_continued_twice                                0        85
    letters_cut_by_tile_end                             3613       992
    letters_slow_piece_wraps                           51964      3917
    iupac_under_substitution                            3107      4954
    iupac_next_to_substitution                          4389     18420
    iupac_under_copy_chunks                            43886    165778
    event_at_chunk_start                               98582     31587
    event_at_tile_start                                 3248       911
    letters_end_at_chunk_end                           67678     21735
    event_subrun                                     1228641    411075
    event_subrun_empty                                391715    106981
    chunk_wholly_under_letters                         11784     64255
    chunk_without_event                              1741721    633358
    max_events_in_chunk                                   12        12
    max_events_in_chunk_gap                               16        16
    tile_before_origin                                   691        42
    tile_beyond_origin                                   919        60
    tile_straddles_origin                                298        16

    dense_classes (dense_piece)                       before     cases
    reads                                               1974       700
    read_shorter_than_16                                   7       265
    read_several_stretches                               490       140
    stretch_cuts_piece_off_16                              0         0   unreachable, see below
    piece_no_event                                         0        25
    tile_more_than_64_items                             6642      1522
    letters_cut_by_tile_start                           2568       671
    letters_cut_by_tile_end                             1146       361
    letters_above_4                                    65520     27437
    letters_above_16                                    4159      3030
    copy_1_16                                        1415568    292812
    copy_above_16                                         64        47
    copy_cut_by_tile_start                               857       188
    copy_cut_by_tile_end                                 857       188
    iupac_under_copy                                    3554      3940
    iupac_next_to_copy                                 21839     19846
    iupac_under_substitution                            3648      6493
    item_near_origin                                     247        55
    item_across_origin                                    15         4
    item_beyond_origin                                 84512     10544
    substitution_across_origin                        101771     12686

    errlog_classes (k_errlog)                         before     cases
    blocks_5120                                        23488      6000
    blocks_8192                                            0      2453
    blocks_staged                                      22585      7393
    blocks_unstaged                                      903      1060
    block_above_buf                                      903      1039
    name_above_256                                         0        60
    al_0 .. al_3 (least)                              319981     97261
    mis_0 .. mis_15 (least)                             1329       424
    row_name_no_whole_dword                                0         0   unreachable, see below
    rows_unstaged_nl_0 .. _15 (least)                    128      1908
    rows_unstaged_name_below_16                            0         0   unreachable, see below
    len_1_16                                         1328673    450509
    len_above_16                                       30881      5716
    len_q0_r1 .. len_q4_r0 (16 classes, least)          2310       387
    iupac_under_event                                   5518      8914
    window_leaves_linear                                   3        10
    window_leaves_circular                             32816      2971
    event_across_origin                                   10         0
    pos_digits_1                                        3422      1579
    pos_digits_2                                       27811     11221
    pos_digits_3                                      262605     62582
    pos_digits_4                                      939810    291932
    pos_digits_5                                      125906     70911
    pos_digits_6                                           0     18000
    len_digits_1                                     1275738    440824
    len_digits_2                                       83812     15108
    len_digits_3                                           4        74
    len_digits_4                                           0       219
    n_ev_multiple_of_64                                   85        27
    piece_no_event                                         0       275
    read_several_aligned_pieces                           92       102

Classes no batch can reach, and why:
  * tile_cut_inside_chunk, tile_64_events_at_one_offset, class_word_carry, tile_mid_piece_chunk0_before_M0 (first pass): they need 64
    events in one 16-byte chunk; the aligned chain yields at most two per output byte (test_aligned_chain_never_packs_a_chunk).  They
    are live in the second pass of -k (MAT_HP_FINAL), whose events are homopolymer edits: tests/test_gpu_hp_edges.py and
    test_dense_homopolymer_edits_take_the_slow_tiles cover that pass; its edit list is no part of an oracle batch, so no census.
  * stretch_cuts_piece_off_16 (dense_piece's m_lo & 15): only batches of unaligned reads take the dense kernel, an unaligned read is
    ONE piece behind no head (oracle/ns_oracle.c: n_pieces = 1), so a stretch starts at a multiple of 4096 of its piece.  The gaps of
    chimeric reads, which one might expect here, take the tile loop of k_materialise (piece_gap above).
  * row_name_no_whole_dword (k_errlog's `d1 > d0` false) and a name shorter than 16 in the row-per-lane copy: a read name is at least
    "<chromosome>_<pos>_aligned_<n>_F_<head>_<len>_<tail>", more than 16 characters.
Counted, in no case's list: event_across_origin (an error-profile event whose own bases straddle the origin: 10 rows before, none here)
is no branch of its own — such a row takes the per-byte loop because its window leaves the chromosome (window_leaves_circular), and
ref_base_at wraps every position beyond the origin, which all rows of a wrapped piece behind the origin exercise.
Input limits: the loader takes chromosome names of any length (ns_set_reference copies the blob; a read name is a uint16 count), the
oracle composes a read name in 4096 bytes: the long-name reference stays non-chimeric, its longest name is 278 characters."""
import copy
import os

import numpy as np
import pytest

from nanosim_amd import engine as E
from nanosim_amd import model as M
from nanosim_amd import synth
from tests import kernel_classes as K
from tests import oracle_lib as O
from tests.test_gpu_parity import compare

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PREFIX = os.path.join(GOLDEN, "model_small", "training")
SEED = 0x5EEDC1A55E5
REACH_MIN = 4
UNALIGNED = E.NS_KIND_UNALIGNED

PHI = ["record:phi_%d" % i for i in range(16)]
UNSTAGED_NL = ["errlog:rows_unstaged_nl_%d" % i for i in range(16)]
STAGED_GRID = ["errlog:mis_%d" % i for i in range(16)] + ["errlog:al_%d" % i for i in range(4)]
LEN_GRID = ["errlog:len_q%d_r%d" % (q, r) for q in range(4) for r in range(4) if q or r] + ["errlog:len_q4_r0"]
LETTERS_8 = ["record:letters_8_at_%d" % i for i in range(4)]

# (id, reference, model, parameters, the classes the case exists for: "<census>:<counter>")
CASES = [
    # pieces and reads shorter than one chunk, pieces without events
    ("tiny-fasta", "small", "small", dict(n_reads=300, median_len=20, sd_len=0.8, min_len=1, emit_errlog=True),
     ["record:piece_shorter_than_16", "record:piece_no_event", "errlog:piece_no_event", "record:strand_forward", "record:strand_reverse"] + PHI),
    ("tiny-fastq-chimeric", "small", "small", dict(n_reads=300, median_len=20, sd_len=0.8, min_len=1, fastq=True, chimeric=True, emit_errlog=True),
     ["record:piece_shorter_than_16", "record:piece_no_event", "record:piece_gap", "errlog:read_several_aligned_pieces"]),
    ("tiny-unaligned", "small", "small", dict(n_reads=300, kind=UNALIGNED, median_len=5, sd_len=1.0, min_len=1, fastq=True),
     ["dense:read_shorter_than_16", "dense:piece_no_event"]),
    # rare errors, matches of hundreds of bases: tiles and whole chunks without an event
    ("clean-fasta", "small", "clean", dict(n_reads=200, emit_errlog=True),
     ["record:tile_cnt_0", "record:tile_cnt_1_62", "record:chunk_without_event", "record:tile_nc_128", "record:tile_L0_start"]),
    ("clean-fastq", "small", "clean", dict(n_reads=200, fastq=True), ["record:tile_cnt_0", "record:tile_nc_above_64"]),
    # insertions with a tail up to NS_EV_LEN_MAX: payloads over several tiles, chunks wholly under letters, 3- and 4-digit lengths, one
    # block above 5 120 bytes in a batch whose average picks k_errlog<5120>
    ("long-payloads-fasta", "small", "long_ins", dict(n_reads=300, max_len=10 ** 6, emit_errlog=True),
     ["record:payload_continued", "record:payload_continued_twice", "record:payload_continued_beyond_tile", "record:letters_cut_by_tile_end",
      "record:chunk_wholly_under_letters", "record:letters_above_16", "record:letters_9_16", "record:tile_L0_ins", "errlog:len_digits_3",
      "errlog:len_digits_4", "errlog:blocks_5120", "errlog:block_above_buf", "errlog:len_above_16"]),
    ("long-payloads-fastq", "small", "long_ins", dict(n_reads=200, max_len=10 ** 6, fastq=True, chimeric=True),
     ["record:payload_continued_twice", "record:chunk_wholly_under_letters", "record:piece_gap"]),
    # the dense model: tiles that end early on a chunk boundary, every event class of the tile loop
    ("dense-fastq", "small", "dense", dict(n_reads=150, fastq=True, emit_errlog=True),
     ["record:tile_cnt_63", "record:tile_cut_on_chunk_boundary", "record:event_at_chunk_start", "record:event_at_tile_start",
      "record:letters_end_at_chunk_end", "record:event_subrun_empty", "record:event_subrun", "record:letters_1_7", "record:tile_L0_mis",
      "record:tile_L0_ins", "record:tile_L0_del", "record:tile_first_A0_negative", "record:tile_last_chunk_partial",
      "errlog:n_ev_multiple_of_64", "errlog:len_1_16", "errlog:len_digits_1", "errlog:len_digits_2", "errlog:pos_digits_1", "errlog:pos_digits_2",
      "errlog:pos_digits_3", "errlog:pos_digits_4", "errlog:blocks_staged"] + LETTERS_8 + LEN_GRID + STAGED_GRID),
    # chromosome names of 60, 120 .. 132 and 270 / 278 characters: k_errlog<8192> staged, its blocks above BUF (row-per-lane stores, the
    # name copy at every nl & 15), names out of LDS
    ("long-names", "names", "small", dict(n_reads=200, emit_errlog=True),
     ["errlog:blocks_8192", "errlog:blocks_staged", "errlog:blocks_unstaged", "errlog:block_above_buf", "errlog:name_above_256"] + UNSTAGED_NL),
    # an ambiguity code every ~20 bases: under substitutions, copied sub-runs and error-profile windows
    ("iupac-aligned", "iupac", "small", dict(n_reads=200, fastq=True, emit_errlog=True),
     ["record:iupac_under_substitution", "record:iupac_next_to_substitution", "record:iupac_under_copy_chunks", "errlog:iupac_under_event"]),
    ("iupac-chimeric", "iupac", "chim", dict(n_reads=150, chimeric=True, emit_errlog=True),
     ["record:iupac_under_copy_chunks", "record:piece_gap", "record:event_at_piece_end", "errlog:iupac_under_event"]),
    ("iupac-unaligned", "iupac", "dense", dict(n_reads=150, kind=UNALIGNED),
     ["dense:iupac_under_copy", "dense:iupac_next_to_copy", "dense:iupac_under_substitution", "dense:copy_above_16", "dense:tile_more_than_64_items",
      "dense:letters_cut_by_tile_start", "dense:letters_cut_by_tile_end", "dense:copy_cut_by_tile_end", "dense:letters_above_4",
      "dense:letters_above_16", "dense:read_several_stretches"]),
    # events within 16 bases of a chromosome end: a linear reference of short contigs, and the circular one
    ("contig-ends", "contigs", "dense", dict(n_reads=300, median_len=200, sd_len=0.4, emit_errlog=True), ["errlog:window_leaves_linear"]),
    ("origin-aligned", "circ", "small", dict(n_reads=150, fastq=True, emit_errlog=True),
     ["errlog:window_leaves_circular", "record:tile_before_origin", "record:tile_beyond_origin",
      "record:tile_straddles_origin", "record:letters_slow_piece_wraps"]),
    ("origin-unaligned", "circ", "small", dict(n_reads=250, kind=UNALIGNED, median_len=4000, sd_len=0.4),
     ["dense:item_near_origin", "dense:item_across_origin", "dense:item_beyond_origin", "dense:substitution_across_origin"]),
    # a handful of reads of ~200 kb: 6-digit positions in the error profile
    ("long-reads", "long", "small", dict(n_reads=6, median_len=200000, sd_len=0.05, emit_errlog=True), ["errlog:pos_digits_5", "errlog:pos_digits_6"]),
]
# the three deletion-heavy models of test_aligned_chain_never_packs_a_chunk: trans -> del, P(match length 0)
DEL_MODELS = dict(del60=((0.2, 0.2, 0.6), 0.7), del80=((0.1, 0.1, 0.8), 0.8), del94=((0.03, 0.03, 0.94), 0.9))
NAME_LENGTHS = (60, 120, 124, 128, 132, 270, 278)
BINS15 = ((0, 1), (1, 2), (2, 3), (3, 5), (5, 7), (7, 10), (10, 14), (14, 19), (19, 25), (25, 33), (33, 45), (45, 60), (60, 90), (90, 150), (150, 1500))


def _long_ins(base):
    """the small model with 1.5 % of its insertions uniform in 100 .. NS_EV_LEN_MAX letters (the table is capped at 4095,
    include/nanosim_amd.h), the others geometric with mean 2.5"""
    m = copy.deepcopy(base)
    k = np.arange(1, 4096, dtype=np.float64)
    cdf = 0.985 * (1.0 - (1.0 - 1.0 / 2.5) ** k) + 0.015 * np.clip((k - 99.0) / (4095.0 - 99.0), 0.0, 1.0)
    cdf[-1] = 1.0
    m.mix_cdf[1] = [cdf.copy(), cdf.copy()]            # NS_INS
    return m


def build_models(d):
    """the models of CASES and DEL_MODELS by name; the synthetic ones are written below directory d"""
    def synth_model(name, spec):
        prefix = os.path.join(str(d), name, "training")
        synth.write_model(prefix, spec, write_pkl=False)
        return M.load_model(prefix, chimeric=True, homopolymer=True, fastq=True)
    small = M.load_model(PREFIX, chimeric=True, homopolymer=True, fastq=True)
    out = dict(small=small, long_ins=_long_ins(small))
    out["chim"] = copy.deepcopy(small)                 # 2.5 segments per read on average: gaps in most reads
    out["chim"].segment_mean = 2.5
    out["chim"].nseg_cdf = M.geometric_cdf(1.0 / 2.5, 0)
    out["clean"] = synth_model("clean", synth.SynthModelSpec(
        n_train=3000, seed=21, aligned_median=2500.0, ecdf_rows=1500, mm_bins=BINS15, mm_means=(400.0,) * 15, mm_zero=(0.0,) + (0.02,) * 14,
        fm_mean=300.0))
    # (the model of test_dense_events_and_long_payloads)
    out["dense"] = synth_model("dense", synth.SynthModelSpec(
        n_train=3000, seed=7, aligned_median=2500.0, mis=(3.0, 0.0, 0.3, 0.5), ins=(8.0, 0.9, 0.12, 0.5), dele=(6.0, 0.95, 0.15, 0.5),
        mm_means=(2.0, 2.5, 3.0, 3.0, 3.5, 3.5, 4.0, 4.0), mm_zero=(0.0, 0.3, 0.3, 0.3, 0.3, 0.3, 0.3, 0.3), fm_mean=3.0))
    for name, (tr, mz) in DEL_MODELS.items():
        out[name] = synth_model(name, synth.SynthModelSpec(n_train=3000, seed=11, aligned_median=1500.0, trans=(tr,) * 7, mm_zero=(mz,) * 8,
                                                           mm_means=(3.0,) * 8, fm_mean=3.0))
    return out


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    return build_models(tmp_path_factory.mktemp("kernel_classes"))


def build_refs():
    lens = (400, 450, 520, 600, 700, 850, 1000, 1300)
    return dict(
        small=M.read_fasta(os.path.join(GOLDEN, "genome_small.fa"), "linear"),
        circ=M.read_fasta(os.path.join(GOLDEN, "genome_circ.fa"), "circular"),
        iupac=M.make_reference(["iupac"], [synth.synth_sequence(60000, 31, iupac_frac=0.05)], "linear"),
        contigs=M.make_reference(["ctg%d" % i for i in range(len(lens))], [synth.synth_sequence(n, 40 + i) for i, n in enumerate(lens)], "linear"),
        names=M.make_reference(["n%03d-" % n + "x" * (n - 5) for n in NAME_LENGTHS],
                               [synth.synth_sequence(20000, 50 + i, iupac_frac=0.0005) for i in range(len(NAME_LENGTHS))], "linear"),
        long=M.make_reference(["long"], [synth.synth_sequence(300000, 60, iupac_frac=0.0002)], "linear"))


@pytest.fixture(scope="module")
def refs():
    return build_refs()


def _params(rname, case, refs):
    kw = dict(seed=SEED, first_read=0, max_len=int(refs[rname].max_chrom))
    kw.update(case)
    return E.make_params(**kw)


_ORACLE = {}


def oracle_case(cid, rname, mname, case, models, refs):
    """(params, oracle batch, census by name) of one case, computed once for both halves"""
    if cid not in _ORACLE:
        p = _params(rname, case, refs)
        big = mname == "long_ins" or rname == "long" or (p.kind == UNALIGNED and mname != "small")
        exp = O.generate(models[mname], refs[rname], p, bytes_per_read=600000 if big else 60000, events_per_read=60000 if big else 8000)
        _ORACLE[cid] = (p, exp, census(exp, refs[rname], p))
    return _ORACLE[cid]


def census(exp, ref, p):
    out = {}
    if p.kind == UNALIGNED:
        out["dense"] = K.dense_classes(exp, ref, p)
    else:
        out["record"] = K.record_classes(exp, ref, p)
        if p.emit_errlog:
            out["errlog"] = K.errlog_classes(exp, ref, p)
    return out


@pytest.mark.parametrize("cid,rname,mname,case,reach", CASES, ids=[c[0] for c in CASES])
def test_cases_reach_their_classes(models, refs, cid, rname, mname, case, reach):
    """every case reaches the classes it exists for, REACH_MIN times at least, on the oracle alone; and all its reads are produced"""
    p, exp, cen = oracle_case(cid, rname, mname, case, models, refs)
    assert len(exp["reads"]) == p.n_reads and not exp["reads"]["flags"].any()
    for entry in reach:
        which, name = entry.split(":")
        assert cen[which].get(name, 0) >= REACH_MIN, "case %s reaches %s %d times (census %s)" % (cid, entry, cen[which].get(name, 0), cen[which])
    if cid == "long-payloads-fasta":           # the block above 5 120 bytes lies in a batch whose AVERAGE row picks the small buffer
        assert cen["errlog"]["blocks_8192"] == 0
    if cid == "long-names":
        assert cen["errlog"]["blocks_5120"] == 0


CUT_CLASSES = ("tile_cut_inside_chunk", "tile_64_events_at_one_offset", "class_word_carry", "tile_mid_piece_chunk0_before_M0")


def _first_pass_cases(models, refs):
    for cid, rname, mname, case, reach in CASES:
        if case.get("kind", E.NS_KIND_ALIGNED) != UNALIGNED:
            p, exp, cen = oracle_case(cid, rname, mname, case, models, refs)
            yield cid, cen["record"]
    for mname in DEL_MODELS:
        for fq in (False, True):
            cid = "%s-%s" % (mname, "fastq" if fq else "fasta")
            if cid not in _ORACLE:
                p = _params("small", dict(seed=4711, n_reads=150, fastq=fq, emit_errlog=True), refs)
                exp = O.generate(models[mname], refs["small"], p, bytes_per_read=80000, events_per_read=40000)
                _ORACLE[cid] = (p, exp, census(exp, refs["small"], p))
            yield cid, _ORACLE[cid][2]["record"]


def test_aligned_chain_never_packs_a_chunk(models, refs):
    """error_list never lets two zero-length matches follow each other (S:1900-1901, oracle/ns_oracle.c: `if (prev_match == 0 && step ==
    0) step = 1`): between two events without an output byte of their own (deletions, whose first output offset is the next byte's) lies
    at least one match base or one event that emits letters, so the aligned chain yields at most two events per output byte and a 16-byte
    chunk holds at most 32 — whatever the model: the three deletion-heavy ones (P(del) 0.6 .. 0.94, P(match 0) 0.7 .. 0.9) stay far
    below.  The gaps of chimeric reads come from the unaligned chain, one event per base at most.

    What follows for materialise_piece's first pass (MAT_REF, MAT_HP_SCRATCH): a tile is cut INSIDE a chunk (M1 = os63) only when 64
    events start in the 16 bytes behind M0, so that cut, the class-word carry it feeds, the mid-piece tile whose chunk 0 starts in front
    of M0 and the `M1 <= M0` hand-over to the slow queue (64 events at ONE offset) are dead code there; no parity test can reach them,
    and they are live only in MAT_HP_FINAL.  A chain change that breaks the rule turns these four untested branches live: this test
    fails first."""
    seen = 0
    for cid, rec in _first_pass_cases(models, refs):
        assert rec["max_events_in_chunk"] <= 32 and rec["max_events_in_chunk_gap"] <= 32, (cid, rec["max_events_in_chunk"], rec["max_events_in_chunk_gap"])
        for name in CUT_CLASSES:
            assert rec[name] == 0, (cid, name, rec[name])
        seen += 1
    assert seen >= 6 + 10
    dense = [rec for cid, rec in _first_pass_cases(models, refs) if cid.startswith("del")]
    assert min(r["tile_cnt_63"] for r in dense) >= REACH_MIN            # (the deletion-heavy models do fill their tiles)


def _check_replay(cid, p, exp, ref):
    if p.kind != UNALIGNED:
        for r, seq, pc, pq, phi in K.record_pieces(exp, p):
            assert exp["records"][seq - 1] == 10                                             # the sequence line starts behind the header line
            os_, pl, ty, ln, epos, rp = K._events(exp, pc)
            out_len, n = int(pc["out_len"]), len(os_)
            at, ev = 0, 0
            for t in K.piece_tiles(os_, pl, ty, rp, out_len, phi, K._Span(ref, pc)):
                assert t["M0"] == at and t["M0"] < t["M1"] <= out_len, (cid, t)              # the tiles partition [0, out_len)
                assert t["jb"] == ev and 0 <= t["cnt"] <= (n if t["queued"] == "stuck" else 63), (cid, t)
                taken = os_[ev:ev + t["cnt"]]
                assert np.all((taken >= t["M0"]) & (taken < t["M1"])), (cid, t)              # ... and take the events that start inside them
                assert (t["A0"] - phi) % 16 == 0 and t["A0"] <= t["M0"] < t["A0"] + 16 or t["queued"] == "stuck", (cid, t)
                at, ev = t["M1"], ev + t["cnt"]
            # every event by exactly one tile; one at the very end of the piece (a trailing deletion) emits nothing and is taken by none
            assert at == out_len and np.all(os_[ev:] == out_len) and not pl[ev:].any(), (cid, at, out_len, ev, n)
    if p.emit_errlog and p.kind == E.NS_KIND_ALIGNED:
        log, rec = exp["errlog"], exp["records"]
        assert K.errlog_classes(exp, ref, p)["predicted_bytes"] == len(log)
        off = 0
        for ri, nl, plist in K.errlog_rows(exp, p):
            ro = int(exp["reads"]["rec_off"][ri])
            name = rec[ro + 1:ro + 1 + nl].tobytes()
            for pc, rows in plist:
                ends = off + np.cumsum(rows)
                assert np.all(log[ends - 1] == 10), (cid, ri)                                # every predicted row ends a line of the image
                starts = ends - rows
                assert log[starts[0]:starts[0] + nl].tobytes() == name and log[starts[-1]:starts[-1] + nl].tobytes() == name if len(rows) else True
                off = int(ends[-1]) if len(rows) else off
        assert off == len(log)
        assert int(np.count_nonzero(log == 10)) == sum(len(rows) for _, _, plist in K.errlog_rows(exp, p) for _, rows in plist)
    if p.kind == UNALIGNED:
        d = K.dense_classes(exp, ref, p)
        assert d["stretches"] == int(np.maximum(1, -(-exp["reads"]["seq_len"].astype(np.int64) // K.DENSE_SEG)).sum())
        assert d["stretch_cuts_piece_off_16"] == 0 and int(exp["reads"]["n_pieces"].max()) == 1 and not exp["reads"]["head"].any()


@pytest.mark.parametrize("cid,rname,mname,case,reach", CASES, ids=[c[0] for c in CASES])
def test_replay_self_check(models, refs, cid, rname, mname, case, reach):
    """the replay against the batch itself: the tiles of every piece partition [0, out_len), every event is taken by exactly one tile
    (or one queued tile), the predicted error-profile size is the image's, and every predicted row starts with its read's name and ends
    a line; unaligned reads are one piece behind no head, so a dense stretch starts at a multiple of 4096 of its piece"""
    p, exp, cen = oracle_case(cid, rname, mname, case, models, refs)
    _check_replay(cid, p, exp, refs[rname])


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


@pytest.mark.gpu
@pytest.mark.parametrize("cid,rname,mname,case,reach", CASES, ids=[c[0] for c in CASES])
def test_gpu_kernel_classes_equal_oracle(engines, models, refs, cid, rname, mname, case, reach):
    p, exp, cen = oracle_case(cid, rname, mname, case, models, refs)
    for entry in reach:
        which, name = entry.split(":")
        assert cen[which].get(name, 0) >= REACH_MIN, (cid, entry)
    eng = engines(rname)
    eng.load_model(models[mname])
    b = eng.generate(p)
    compare(b, exp, p)
