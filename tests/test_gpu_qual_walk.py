"""GPU parity on quality tables the Python loader would have snapped: buckets with several thresholds, whose draws the bucket look-ups
must walk (qual_value_lut) or redo by binary search for the whole wavefront (qual_lookup16).  Tables a caller of the C ABI may pass as
they are (include/nanosim_amd.h: qual_thr is any non-decreasing table).

Two table sets, loaded through Engine.load_model; the oracle reads the same tables:
  raw   the closed-form tables of the small model (quality_thresholds, unsnapped): four to six flagged buckets per class, in the tails;
  walk  tests/test_qual_probe.py walk_tables(): 63 flagged buckets per class, and per class quality levels that only the walk can emit
        and that no other class emits at all.  Where such a level appears in a batch's quality lines, the walk ran for that class.

Every FASTQ path is taken: aligned reads (k_qualities: match, substituted, inserted), head and tail (ht), unaligned reads and chimeric
gaps (k_materialise_dense: unmapped), --perfect, -k 5 (the homopolymer record pass), the r9_like operating point (the slow-tile queue),
transcriptome reads with polyA tails (ht) and --uracil, metagenome reads.  Records, error profile and polyA lengths equal the oracle's
byte for byte."""
import copy
import os

import numpy as np
import pytest

from nanosim_amd import engine as E
from nanosim_amd import metagenome as MG
from nanosim_amd import model as M
from nanosim_amd import synth
from nanosim_amd import transcriptome as T
from tests import oracle_lib as O
from tests.test_gpu_operating_points import T_OUT, TILE_EVENTS, _window_counts
from tests.test_gpu_parity import compare
from tests.test_qual_probe import Q_HT, Q_INS, Q_MATCH, Q_MIS, Q_UNMAPPED, flagged, walk_only_levels, walk_tables

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PREFIX = os.path.join(GOLDEN, "model_small", "training")
SETS = ("raw", "walk")
ALIGNED_CLASSES = (Q_MATCH, Q_MIS, Q_INS, Q_HT)


def with_tables(m, which):
    """a copy of model m whose quality tables are the raw or walk set"""
    out = copy.copy(m)
    out._keep = []
    if which == "raw":
        out.qual_thr = np.stack([M.quality_thresholds(*m.quals[nm]) for nm in M.NS_Q_NAMES])
    else:
        out.qual_thr = np.stack(walk_tables())
    assert all(flagged(t).any() for t in out.qual_thr)
    return out


def quality_levels(records):
    """the quality levels (byte - 33) of every quality line of a FASTQ record blob"""
    lines = bytes(records).split(b"\n")
    assert lines[-1] == b"" and len(lines) % 4 == 1 and all(ln.startswith(b"@") for ln in lines[0:-1:4])
    q = np.frombuffer(b"".join(lines[3::4]), dtype=np.uint8).astype(np.int64) - 33
    assert len(q) and q.min() >= 0
    return np.bincount(q, minlength=128)


def check(b, exp, p, which, classes, polya=None):
    compare(b, exp, p)
    if polya is not None:
        assert np.array_equal(b.polya(), polya)
    if which == "walk":
        lv = quality_levels(b.records())
        for c in classes:
            n = int(lv[walk_only_levels(c)].sum())
            assert n > 0, "no walk-only level of class %s in the quality lines" % M.NS_Q_NAMES[c]


@pytest.fixture(scope="module")
def genome_models(small_model):
    return {w: with_tables(small_model, w) for w in SETS}


GENOME_CASES = [
    ("aligned", dict(n_reads=300, fastq=True, emit_errlog=True), ALIGNED_CLASSES),
    ("unaligned", dict(kind=E.NS_KIND_UNALIGNED, n_reads=300, fastq=True), (Q_UNMAPPED,)),
    ("chimeric", dict(n_reads=600, chimeric=True, fastq=True, emit_errlog=True), ALIGNED_CLASSES + (Q_UNMAPPED,)),
    ("perfect", dict(kind=E.NS_KIND_PERFECT, n_reads=300, fastq=True), (Q_MATCH,)),
    ("k5", dict(n_reads=300, kmer_bias=5, fastq=True, emit_errlog=True), ALIGNED_CLASSES),
    ("k5_chimeric", dict(n_reads=200, kmer_bias=5, chimeric=True, fastq=True), ALIGNED_CLASSES),
]


@pytest.mark.parametrize("which", SETS)
def test_genome_fastq_with_flagged_buckets(genome_models, small_ref, which):
    mdl = genome_models[which]
    e = E.Engine(0)
    try:
        e.set_reference(small_ref)
        e.load_model(mdl)
        for name, case, classes in GENOME_CASES:
            p = E.make_params(**dict(dict(seed=0x9A11E7, first_read=11, max_len=small_ref.max_chrom), **case))
            b = e.generate(p)
            exp = O.generate(mdl, small_ref, p)
            try:
                check(b, exp, p, which, classes)
            except AssertionError as err:
                raise AssertionError("%s tables, %s: %s" % (which, name, err)) from None
            rd = b.reads()
            if name == "aligned":
                assert int((rd["head"].astype(np.int64) + rd["tail"]).sum()) > 1000, "too few head / tail bases"
            if name == "chimeric":
                assert np.any(b.pieces()["kind"] != 0), "no chimeric gaps"
    finally:
        e.close()


@pytest.mark.parametrize("which", SETS)
def test_r9_like_fastq_slow_tiles_with_flagged_buckets(small_ref, which, tmp_path):
    prefix = str(tmp_path / "training")
    synth.write_model(prefix, synth.operating_point_spec("r9_like"), write_pkl=False)
    mdl = with_tables(M.load_model(prefix, chimeric=True, homopolymer=True, fastq=True), which)
    e = E.Engine(0)
    try:
        e.set_reference(small_ref)
        e.load_model(mdl)
        for case in (dict(fastq=True, emit_errlog=True), dict(chimeric=True, fastq=True)):
            p = E.make_params(seed=0x9A11E8, first_read=0, n_reads=300, max_len=small_ref.max_chrom, **case)
            b = e.generate(p)
            check(b, O.generate(mdl, small_ref, p, **O.sizes_for_model(mdl, p)), p, which, (Q_MATCH, Q_MIS, Q_INS))
            full, _ = _window_counts(b.pieces(), b.events())
            assert len(full) and np.mean(full > TILE_EVENTS) > 0.5, "the slow-tile queue was not reached (tiles of %d bytes)" % T_OUT
    finally:
        e.close()


@pytest.mark.parametrize("which", SETS)
def test_transcriptome_fastq_with_flagged_buckets(which):
    trx = os.path.join(GOLDEN, "trx")
    tr = T.read_transcriptome(os.path.join(trx, "transcripts.fa"), os.path.join(trx, "expression.tsv"), os.path.join(trx, "polya.txt"), "guppy")
    mdl = with_tables(M.load_model(PREFIX, transcriptome=True, fastq=True, homopolymer=True), which)
    e = E.Engine(0)
    try:
        e.set_transcriptome(tr)
        e.load_model(mdl)
        for case, classes in ((dict(n_reads=400, fastq=True, uracil=True, emit_errlog=True), ALIGNED_CLASSES),
                              (dict(n_reads=300, kmer_bias=5, fastq=True, uracil=True), ALIGNED_CLASSES),
                              (dict(n_reads=300, kind=E.NS_KIND_UNALIGNED, fastq=True, min_len=50, max_len=5000), (Q_UNMAPPED,))):
            p = E.make_params(**dict(dict(seed=0x9A11E9, first_read=0, max_len=10 ** 9, trx=True), **case))
            b = e.generate(p)
            exp = O.generate_trx(mdl, tr, p)
            check(b, exp, p, which, classes, polya=exp["polya"])
            if p.kind != E.NS_KIND_UNALIGNED:
                assert int(b.polya().astype(np.int64).sum()) > 100, "too few polyA bases"
    finally:
        e.close()


@pytest.mark.parametrize("which", SETS)
def test_metagenome_fastq_with_flagged_buckets(small_model, which):
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        meta_ref = MG.read_metagenome(os.path.join(GOLDEN, "meta", "genome_list.tsv"), os.path.join(GOLDEN, "meta", "dna_type_list.tsv"))
    finally:
        os.chdir(cwd)
    _, samples = MG.read_abundance(os.path.join(GOLDEN, "meta", "abundance.tsv"), meta_ref.species)
    abun = samples[0]
    infl = {sp: MG.inflate_abun(abun, sp, small_model.abun_inflation) for sp in abun}
    mdl = with_tables(small_model, which)
    e = E.Engine(0)
    try:
        e.set_metagenome(meta_ref, abun, infl)
        e.load_model(mdl)
        for case, classes in ((dict(n_reads=300, fastq=True, emit_errlog=True), ALIGNED_CLASSES),
                              (dict(n_reads=300, chimeric=True, fastq=True), ALIGNED_CLASSES + (Q_UNMAPPED,))):
            p = E.make_params(seed=0x9A11EA, first_read=0, max_len=meta_ref.max_chrom, meta=True, **case)
            b = e.generate(p)
            exp = O.generate_meta(mdl, meta_ref, abun, infl if p.chimeric else None, p)
            check(b, exp, p, which, classes)
            assert np.array_equal(e.species_bases(), exp["species_bases"])
    finally:
        e.close()

