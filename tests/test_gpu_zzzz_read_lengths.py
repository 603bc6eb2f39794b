"""GPU parity of the training side's read-length models ("Read lengths: the KDE inputs"): ns_read_lengths (k_len_scan,
k_len_flag, k_len_reduce, csrc/ns_train.h) against what the REAL src/head_align_tail_dist.py collected
(tests/golden/reference_read_len.json.gz) and against the same walk compiled for the host; and the whole training side end to end — a
prefix this project characterised itself, opened by model.load_model and simulated from."""
import ctypes as C
import gzip
import json
import os

import numpy as np
import pytest

from nanosim_amd import characterize, model
from nanosim_amd import engine as E
from tests.test_read_lengths import (BAD, REF, build_host_walk, check_argument_errors, check_bad_records, check_genome, check_hand_cases,
                                     check_transcriptome, load_fixture, raw_call, rec)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20260926                     # (the parameters of smoke())


@pytest.fixture(scope="module")
def fx():
    return load_fixture()


@pytest.fixture(scope="module")
def host():
    return build_host_walk()


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def host_figures(fx, host):
    """the host walk's figures for both modes, computed once"""
    t = fx["trx"]
    return dict(genome=characterize.count_read_lengths(host, fx["refs"], fx["primary"]),
                trx=characterize.count_read_lengths(host, t["refs"], t["records"], "transcriptome", t["genome_records"]))


def same_as_host(got, want):
    """every array of count_read_lengths, the figures record by record"""
    assert sorted(got) == sorted(want)
    for k, v in want.items():
        if k != "ms_kernel":
            assert got[k].dtype == v.dtype and np.array_equal(got[k], v), k


def test_gpu_fixture_in_both_modes(fx, eng, host_figures):
    """599 records: three workgroups, a read across the first border (records 255 .. 257), a CIGAR of 5 000 ops, the length sort"""
    g = check_genome(eng, fx)
    same_as_host(g, host_figures["genome"])
    assert g["ms_kernel"] > 0
    t = check_transcriptome(eng, fx)
    same_as_host(t, host_figures["trx"])
    assert t["ms_kernel"] > 0
    print("ms_kernel: genome %.3f, transcriptome (two calls) %.3f" % (g["ms_kernel"], t["ms_kernel"]))


def test_gpu_between_generate_calls_and_twice(fx, small_model, small_ref, host_figures):
    p = E.make_params(seed=SEED, first_read=0, n_reads=256, kind=E.NS_KIND_ALIGNED, fastq=True, chimeric=True, max_len=small_ref.max_chrom,
                      emit_errlog=True)
    e = E.Engine(0)
    try:
        e.set_reference(small_ref)
        e.load_model(small_model)
        first = e.generate(p).records().tobytes()
        same_as_host(check_genome(e, fx), host_figures["genome"])
        same_as_host(check_genome(e, fx), host_figures["genome"])
        same_as_host(check_transcriptome(e, fx), host_figures["trx"])
        again = e.generate(p).records().tobytes()
        same_as_host(characterize.count_read_lengths(e, fx["refs"], fx["primary"][:3]), characterize.count_read_lengths(build_host_walk(), fx["refs"], fx["primary"][:3]))
        same_as_host(check_genome(e, fx), host_figures["genome"])
    finally:
        e.close()
    assert first == again and len(first) > 0


def equal_to_host(eng, host, refs, records, read_off=None, mode=0):
    g, h = raw_call(eng, refs, records, read_off, mode), raw_call(host, refs, records, read_off, mode)
    assert g[0] == h[0] == 0 and (g[1].n_segments, g[1].n_bad, g[1].first_bad) == (h[1].n_segments, h[1].n_bad, h[1].first_bad)
    for a, b in zip(g[2:], h[2:]):
        assert np.array_equal(a, b)                           # (the sentinel behind the segments included)
    return g


def test_gpu_smallest_calls(fx, eng, host):
    rc, out, aln, reads, seg = raw_call(eng, REF, [], [0])
    assert rc == 0 and (out.n_segments, out.n_bad, out.first_bad, out.ms_kernel) == (0, 0, 0, 0)
    g = equal_to_host(eng, host, REF, [rec("7S120M3S", 1)])
    assert g[1].n_segments == 1 and g[4][0] == 120 and g[3][0].tolist() == (130, 7, 3, 1) and g[2][0]["edge"] == 1
    recs = [rec("%dS%dM" % (i % 5, 100 + i), 1 + 37 * i, 16 * (i % 2), name="r%d" % i) for i in range(257)]
    g = equal_to_host(eng, host, REF, recs)
    assert g[1].n_segments == 257 and g[4].tolist() == [100 + i for i in range(257)] and (g[3]["n_segments"] == 1).all()
    # 64 and 65 records (index order / the length sort), one read of all of them, and reads that end at a workgroup border
    for n in (64, 65):
        equal_to_host(eng, host, fx["refs"], fx["primary"][:n])
    equal_to_host(eng, host, REF, recs, [0, 257])
    equal_to_host(eng, host, REF, recs, [0, 256, 257])
    equal_to_host(eng, host, REF, recs, [0, 1, 255, 257], mode=1)
    figures = characterize.count_read_lengths(eng, REF, [])
    assert len(figures["aligned_ref_length"]) == 0 and len(figures["head_vs_ht_ratio"]) == 0


def test_gpu_hand_cases_and_bad_records(eng):
    check_hand_cases(eng)
    check_bad_records(eng)
    recs = [rec("50M", name="fine")] * 300 + [rec("50M7", name="culprit")] + [rec("50M", name="fine")] * 10 + [rec("Z", name="second")]
    with pytest.raises(ValueError, match=r"2 SAM record\(s\).*first is record 300 \(culprit\): CIGAR 50M7"):
        characterize.count_read_lengths(eng, REF, recs)
    assert len(BAD) == 17


def test_gpu_argument_checks(eng):
    check_argument_errors(eng, E.NS_EINVAL)
    assert b"ns_read_lengths" in eng.L.ns_last_error(eng.ctx)
    recs = [rec("10M"), rec("20M")]
    cg, cg_off = characterize._pack([r[4] for r in recs])
    arrs = dict(reverse=np.zeros(2, dtype=np.uint8), ref_id=np.zeros(2, dtype=np.uint32), start=np.zeros(2, dtype=np.uint64),
                total=np.array([1000], dtype=np.uint64), read_off=np.array([0, 1, 2], dtype=np.uint64))
    reads, seg = np.zeros(2, dtype=characterize.LEN_READ_DTYPE), np.zeros(2, dtype=np.uint64)
    out = characterize.NsLenResult()
    out.reads, out.segments = reads.ctypes.data, seg.ctypes.data

    def call(ref_id=arrs["ref_id"], n_refs=1, cigar_off=cg_off, extra=(None, None), res=out):
        return eng.L.ns_read_lengths(eng.ctx, cg.ctypes.data, cigar_off.ctypes.data if cigar_off is not None else None, arrs["reverse"].ctypes.data,
                                     ref_id.ctypes.data, arrs["start"].ctypes.data, arrs["total"].ctypes.data, n_refs, arrs["read_off"].ctypes.data, 2, 2, 0,
                                     extra[0], extra[1], C.byref(res) if res is not None else None)
    assert call() == 0 and seg.tolist() == [10, 20] and out.n_segments == 2
    assert call(ref_id=np.array([0, 1], dtype=np.uint32)) == E.NS_EINVAL and b"ref_id of record 1" in eng.L.ns_last_error(eng.ctx)
    assert call(n_refs=0) == E.NS_EINVAL
    assert call(cigar_off=np.array([0, 5, 3], dtype=np.uint64)) == E.NS_EINVAL
    assert call(cigar_off=None) == E.NS_EINVAL
    assert call(extra=(arrs["ref_id"].ctypes.data, None)) == E.NS_EINVAL
    assert call(res=None) == E.NS_EINVAL
    out.reads = None
    assert call() == E.NS_EINVAL
    out.reads = reads.ctypes.data
    extra = np.array([3, 0xffffffff], dtype=np.uint32)
    cg, cg_off = characterize._pack(["5S10M6S", "5S20M6S"])
    assert call(cigar_off=cg_off, extra=(extra.ctypes.data, extra.ctypes.data)) == 0 and reads.tolist() == [(21, 3, 3, 1), (31, 5, 6, 1)]


def test_gpu_end_to_end_a_prefix_characterised_here_loads_and_simulates(fx, eng, small_ref, tmp_path):
    """SAM text -> hist, model_fitting, read_lengths -> model.load_model -> 2 000 simulated reads.  Without read_lengths the prefix has
    no _strandness_rate, no _reads_alignment_rate and no KDE: load_model raises FileNotFoundError.
    The bound on the simulated aligned lengths comes from the KDE itself.  A draw is data[i] + 10 z with z the normal quantile of one of
    2^32 equally spaced probabilities, so |z| < 6.4, cut to an integer: every DRAW lies within 65 bases of a data point — on either side,
    so the sample's floor is min - 65, not min (6 of the 558 data points are 99, the smallest; half of their draws fall below).  A read's
    aligned length is its draw or, when the last step of the error walk runs past the draw, the end of that step (error_list: the walk
    goes on while pos < draw and the length becomes where it stops), so the draw lies behind the read's last error and not behind its
    length: the window [last error + 1 - 65, length + 65] of every read must hold a data point, and no length lies below min - 65.
    (A draw above the longest chromosome is drawn again: the data points above it cannot be met.)"""
    with gzip.open(os.path.join(ROOT, "tests", "golden", "reference_hist.json.gz"), "rt") as f:
        cs = json.load(f)["cs"]
    prefix = str(tmp_path / "training")
    with open(prefix + ".sam", "w") as f:
        f.write(fx["sam"])
    refs, recs, unaligned_len, strandness = characterize.primary_and_unaligned(prefix + ".sam")
    assert recs == fx["primary"]
    with open(prefix + "_primary.sam", "w") as f:           # the reference's <prefix>_primary file as SAM text, a cs tag on every record
        f.write("".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs))
        for i, r in enumerate(recs):
            f.write("%s\t%d\t%s\t%d\t60\t%s\t*\t0\t0\t*\t*\tcs:Z:%s\n" % (r + (cs[i % len(cs)],)))
    assert characterize.length_records(prefix + "_primary.sam") == (refs, recs)
    characterize.hist(prefix, characterize.cs_from_sam(prefix + "_primary.sam"), eng)
    characterize.model_fitting(prefix, eng)
    with pytest.raises(FileNotFoundError):
        model.load_model(prefix)
    figures = characterize.read_lengths(prefix, refs, recs, eng, unaligned_len, strandness)
    assert figures["aligned_ref_length"].tolist() == fx["genome"]["aligned_ref_length"]
    m = model.load_model(prefix)
    assert m.strandness_rate == round(fx["strandness"], 3) and m.alignment_rate == 405 / len(fx["unaligned_len"])
    data = np.array(fx["genome"]["aligned_ref_length"], dtype=np.float64)
    assert np.array_equal(m.kde[model.NS_KDE_ALIGNED][0], data) and m.kde[model.NS_KDE_ALIGNED][1] == 10
    assert np.array_equal(m.kde[model.NS_KDE_HT][0], np.log10(np.array(fx["genome"]["ht_length"]) + 1))
    assert np.array_equal(m.kde[model.NS_KDE_UNALIGNED][0], np.array(fx["unaligned_len"], dtype=np.float64))
    e = E.Engine(0)
    try:
        e.set_reference(small_ref)
        e.load_model(m)
        b = e.generate(E.make_params(seed=SEED, first_read=0, n_reads=2000, kind=E.NS_KIND_ALIGNED, max_len=small_ref.max_chrom))
        reads, pieces, events, n_bytes = b.reads(), b.pieces(), b.events(), len(b.records())
    finally:
        e.close()
    assert len(reads) == 2000 and len(pieces) == 2000 and n_bytes > 2000 * 100 and (reads["seq_len"] > 0).all()
    lengths = pieces["ref_len"].astype(np.int64)
    usable = np.sort(data[data <= small_ref.max_chrom])
    reach = 65
    has = pieces["n_ev"] > 0
    draw_lo = lengths.copy()                                 # the smallest draw the read can come from
    draw_lo[has] = events["pos"][(pieces["ev_off"][has] + pieces["n_ev"][has] - 1).astype(np.int64)].astype(np.int64) + 1
    assert has.sum() > 1900 and (draw_lo <= lengths).all()
    at = np.searchsorted(usable, draw_lo - reach)            # the first data point inside the window, if there is one
    print("aligned lengths %d .. %d, data %d .. %d, windows up to %d wide" % (lengths.min(), lengths.max(), usable[0], usable[-1], (lengths - draw_lo).max() + 2 * reach + 1))
    assert lengths.min() >= usable[0] - reach
    assert (at < len(usable)).all() and (usable[np.minimum(at, len(usable) - 1)] <= lengths + reach).all()
    assert len(np.unique(lengths)) > 500                     # a sample of the data, not one value
