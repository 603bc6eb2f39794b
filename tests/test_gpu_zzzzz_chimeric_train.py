"""GPU parity of the training side's chimeric step ("Chimeric reads: the split-alignment choice"): ns_cigar_spans and
ns_chimeric_select (k_chim_scan, k_chim_select, csrc/ns_train.h) against what the REAL src/get_primary_sam.py collected and wrote
(tests/golden/reference_chimeric_train.json.gz) and against the same walk compiled for the host; and the whole training side end to
end — a prefix this project characterised itself, opened by model.load_model(chimeric=True) and simulated from with --chimeric."""
import ctypes as C
import gzip
import json
import os
import re

import numpy as np
import pytest

from nanosim_amd import characterize, model
from nanosim_amd import engine as EN
from tests import oracle_lib
from tests.test_chimeric_train import (BAD_CIGARS, CIRCULAR, HAND, SPECIES, E, build_host_walk, call, check_bad, check_cigar_bleed, check_circular, check_fixture, check_hand,
                                       check_mask_borders, load_fixture, many_compatible, many_overlapping, sam_file)

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
    e = EN.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def host_choice(fx, host, tmp_path_factory):
    """the host walk's results on the fixture in both species settings, computed once"""
    return check_fixture(host, fx, tmp_path_factory.mktemp("host"))


def same_choice(got, want):
    assert sorted(got) == sorted(want)
    for k, v in want.items():
        if k.startswith("ms_"):
            continue
        if isinstance(v, np.ndarray):
            assert got[k].dtype == v.dtype and np.array_equal(got[k], v), k
        else:
            assert got[k] == v, k


def equal_to_host(eng, host, reads, **kw):
    g, h = call(eng, reads, **kw), call(host, reads, **kw)
    assert g.reads == h.reads and (g.n_gaps, g.pos_strand, g.n_bad, g.first_bad, g.count) == (h.n_gaps, h.pos_strand, h.n_bad, h.first_bad, h.count)
    assert np.array_equal(g.ent, h.ent) and np.array_equal(g.ent_off, h.ent_off)
    return g


def test_gpu_fixture_in_both_species_settings(fx, eng, host_choice, tmp_path):
    """300 reads, 463 entries: two workgroups of k_chim_scan and of k_chim_select, both visiting orders"""
    got = check_fixture(eng, fx, tmp_path)
    for key in ("genome", "meta"):
        same_choice(got[key], host_choice[key])
        assert got[key]["ms_kernel"] > 0 and 0 < got[key]["ms_scan"] <= got[key]["ms_kernel"] and got[key]["ms_spans"] > 0
    print("ms_kernel %.3f (scan %.3f), spans %.3f" % (got["genome"]["ms_kernel"], got["genome"]["ms_scan"], got["genome"]["ms_spans"]))


def test_gpu_smallest_calls_and_read_counts(eng, host):
    r = call(eng, [])
    assert (r.n_gaps, r.pos_strand, r.n_bad, r.first_bad, r.count) == (0, 0, 0, 0, [[0, 0], [0, 0]])
    assert equal_to_host(eng, host, [[E("7S120M3S")]]).reads == [(1, characterize.CHIM_POS_STRAND, [(0, 1, -1)])]
    assert equal_to_host(eng, host, [[E("100M80S"), E("130S50M", 1)]]).reads == [(2, characterize.CHIM_HAS_SA | characterize.CHIM_POS_STRAND, [(0, 1, -1), (1, 0, 30)])]
    # the wavefront and workgroup borders: reads of 1, 2 or 3 entries by turns, reverse and forward
    def read(i):
        p = E("%dM%dS" % (100 + i % 7, 400), i % 3, 1000 + i, nm=i % 5, rev=bool(i % 2))
        return [p] + [E("%dS%dM" % (120 + 150 * k + i % 11, 100), (i + k) % 3, 50000 + 1000 * k + i, nm=k) for k in range(i % 3)]
    for n in (63, 64, 65, 255, 256, 257):
        g = equal_to_host(eng, host, [read(i) for i in range(n)])
        assert [k for k, _, _ in g.reads] == [1 + i % 3 for i in range(n)] and g.n_gaps == sum(i % 3 for i in range(n))
        assert g.pos_strand == sum(1 for i in range(n) if i % 2 == 0)


@pytest.mark.parametrize("n", [63, 64, 65, 130])
def test_gpu_reads_at_the_mask_word_borders(eng, host, n):
    check_mask_borders(eng, n)
    lone = [E("100M")]
    equal_to_host(eng, host, [lone, many_compatible(n)[0], many_overlapping(n, n), many_overlapping(n, 1)] + [lone] * 70 + [many_compatible(n)[0]])


def test_gpu_hand_made_reads(eng, host):
    for case in HAND:
        check_hand(eng, case)
    for case in CIRCULAR:
        check_circular(eng, case)
    equal_to_host(eng, host, [c[1] for c in HAND])             # all of them in one call
    equal_to_host(eng, host, [c[1] for c in CIRCULAR], ref_total=(5000, 5000, 10 ** 9))


def test_gpu_bad_cigars(eng, host):
    for bad in BAD_CIGARS:
        check_bad(eng, bad)
    check_cigar_bleed(eng)
    cigars = ["50M"] * 300 + ["50M7"] + ["%dS50M" % i for i in range(10)] + ["Z"]
    got, n_bad, first_bad, ms = characterize.cigar_spans(eng, cigars)
    want = characterize.cigar_spans(host, cigars)
    assert (n_bad, first_bad) == (2, 300) == want[1:3] and np.array_equal(got, want[0]) and ms > 0


def test_gpu_argument_checks(eng):
    cg, cg_off = characterize._pack(["10M", "20M", "5S7M"])
    arrs = dict(ent_off=np.array([0, 1, 3], dtype=np.uint64), ref_id=np.zeros(3, dtype=np.uint32), start=np.array([10, 500, 900], dtype=np.uint64),
                nm=np.zeros(3, dtype=np.uint32), reverse=np.zeros(3, dtype=np.uint8), total=np.array([10 ** 6], dtype=np.uint64), species=np.zeros(1, dtype=np.uint32))
    pieces, reads = np.zeros(3, dtype=characterize.CHIM_PIECE_DTYPE), np.zeros(2, dtype=characterize.CHIM_READ_DTYPE)
    count = np.zeros(2, dtype=np.uint64)
    out = characterize.NsChimResult()
    out.pieces, out.reads, out.species_count = pieces.ctypes.data, reads.ctypes.data, count.ctypes.data

    def sel(ent_off=arrs["ent_off"], ref_id=arrs["ref_id"], species=arrs["species"], n_refs=1, n_species=1, cigar_off=cg_off, res=out, n_reads=2):
        return eng.L.ns_chimeric_select(eng.ctx, cg.ctypes.data, cigar_off.ctypes.data if cigar_off is not None else None, ent_off.ctypes.data, n_reads,
                                        ref_id.ctypes.data, arrs["start"].ctypes.data, arrs["nm"].ctypes.data, arrs["reverse"].ctypes.data, arrs["total"].ctypes.data,
                                        species.ctypes.data, n_refs, n_species, C.byref(res) if res is not None else None)
    err = lambda: eng.L.ns_last_error(eng.ctx)
    assert sel() == 0 and reads.tolist() == [(1, 1), (1, 5)] and (out.n_gaps, out.pos_strand, out.n_bad, out.first_bad) == (0, 2, 0, 3)
    assert sel(ref_id=np.array([0, 0, 1], dtype=np.uint32)) == EN.NS_EINVAL and b"ref_id of entry 2" in err() and b"ns_chimeric_select" in err()
    assert sel(n_refs=0) == EN.NS_EINVAL
    assert sel(species=np.array([1], dtype=np.uint32)) == EN.NS_EINVAL and b"species of reference 0" in err()
    assert sel(n_species=0) == EN.NS_EINVAL
    assert sel(ent_off=np.array([0, 0, 3], dtype=np.uint64)) == EN.NS_EINVAL and b"read 0 has no entry" in err()
    assert sel(ent_off=np.array([0, 3, 2], dtype=np.uint64)) == EN.NS_EINVAL and b"decreases at read 1" in err()
    assert sel(ent_off=np.array([1, 2, 3], dtype=np.uint64)) == EN.NS_EINVAL
    assert sel(cigar_off=np.array([0, 5, 3, 9], dtype=np.uint64)) == EN.NS_EINVAL
    assert sel(cigar_off=None) == EN.NS_EINVAL and sel(res=None) == EN.NS_EINVAL
    out.reads = None
    assert sel() == EN.NS_EINVAL
    out.reads = reads.ctypes.data
    assert sel(n_reads=0, ent_off=np.array([0], dtype=np.uint64)) == 0 and out.first_bad == 0
    spans = np.zeros(3, dtype=characterize.CHIM_ENT_DTYPE)
    n_bad, first_bad, ms = C.c_uint64(9), C.c_uint64(9), C.c_double(9)
    span = lambda off=cg_off, res=spans.ctypes.data, nb=C.addressof(n_bad): eng.L.ns_cigar_spans(eng.ctx, cg.ctypes.data, off.ctypes.data if off is not None else None, 3,
                                                                                                 res, nb, C.addressof(first_bad), C.addressof(ms))
    assert span() == 0 and spans.tolist() == [(0, 10, 10, 10), (0, 20, 20, 20), (5, 12, 7, 7)] and (n_bad.value, first_bad.value) == (0, 3)
    assert span(off=np.array([0, 5, 3, 9], dtype=np.uint64)) == EN.NS_EINVAL and b"ns_cigar_spans" in err()
    assert span(off=None) == EN.NS_EINVAL and span(res=None) == EN.NS_EINVAL and span(nb=None) == EN.NS_EINVAL


def test_gpu_between_generate_calls_and_twice(fx, small_model, small_ref, host_choice, tmp_path):
    p = EN.make_params(seed=SEED, first_read=0, n_reads=256, kind=EN.NS_KIND_ALIGNED, fastq=True, chimeric=True, max_len=small_ref.max_chrom,
                       emit_errlog=True)
    refs, records, _, _ = characterize.chimeric_records(sam_file(fx, tmp_path))
    e = EN.Engine(0)
    try:
        e.set_reference(small_ref)
        e.load_model(small_model)
        first = e.generate(p).records().tobytes()
        same_choice(characterize.select_chimeric(e, refs, records), host_choice["genome"])
        same_choice(characterize.select_chimeric(e, refs, records), host_choice["genome"])
        same_choice(characterize.select_chimeric(e, refs, records, SPECIES), host_choice["meta"])
        again = e.generate(p).records().tobytes()
        same_choice(characterize.select_chimeric(e, refs, records), host_choice["genome"])
    finally:
        e.close()
    assert first == again and len(first) > 0


def with_cs_and_qual(sam: str, cs: list) -> str:
    """the fixture's SAM text with what hist and base_qualities read on top: a cs:Z tag on every aligned record (those of the histogram
    fixture, by turns) and a QUAL — and a SEQ — as long as the record's soft clips plus the bases its cs string covers"""
    rng = np.random.default_rng(11)
    quals = lambda n: bytes(rng.integers(35, 74, n, dtype=np.uint8)).decode()          # Phred 2 .. 40: no quality of 0
    out, k = [], 0
    for l in sam.splitlines(True):
        if l.startswith("@"):
            out.append(l)
            continue
        f = l.rstrip("\n").split("\t")
        if int(f[1]) & 4:
            if f[9] != "*":
                f[10] = quals(len(f[9]))
        else:
            c = cs[k % len(cs)]
            k += 1
            covered = sum(int(n) for n in re.findall(r":(\d+)", c)) + len(re.findall(r"\*[a-z][a-z]", c)) + sum(len(s) for s in re.findall(r"\+([a-z]+)", c))
            head, tail = characterize._CLIP_HEAD.match(f[5]), characterize._CLIP_TAIL.search(f[5])      # (the clips quals_from_sam takes off)
            n = covered + (int(head.group(1)) if head else 0) + (int(tail.group(1)) if tail else 0)
            f[9], f[10] = "A" * n, quals(n)
            f.append("cs:Z:" + c)
        out.append("\t".join(f) + "\n")
    return "".join(out)


def test_gpu_end_to_end_a_chimeric_prefix_characterised_here_loads_and_simulates(fx, eng, small_ref, tmp_path):
    """SAM text -> chimeric, then hist, model_fitting, read_lengths and base_qualities on <prefix>_primary.sam -> load_model(chimeric=True)
    -> 3 000 reads of a --chimeric genome run, byte for byte the oracle's on that model.  Without chimeric() the prefix has no
    _chimeric_info: load_model(chimeric=True) raises FileNotFoundError."""
    with gzip.open(os.path.join(ROOT, "tests", "golden", "reference_hist.json.gz"), "rt") as f:
        cs = json.load(f)["cs"]
    prefix = str(tmp_path / "training")
    with open(prefix + ".sam", "w") as f:
        f.write(with_cs_and_qual(fx["sam"], cs))
    refs, recs, unaligned_len, strandness = characterize.chimeric(prefix, prefix + ".sam", eng, pickles=False)
    assert [list(r) for r in recs] == [r[:5] for r in fx["genome"]["written"]] and strandness == fx["genome"]["strandness"]
    assert characterize.length_records(prefix + "_primary.sam") == (refs, recs)
    os.rename(prefix + "_chimeric_info", prefix + "_chimeric_info.aside")
    characterize.hist(prefix, characterize.cs_from_sam(prefix + "_primary.sam"), eng)
    characterize.model_fitting(prefix, eng)
    characterize.read_lengths(prefix, refs, recs, eng, unaligned_len, strandness, pickles=False, merge=True)
    aligned, _ = characterize.quals_from_sam(prefix + "_primary.sam", primary_only=False)
    assert len(aligned) == len(recs) - sum(1 for r in recs if r[1] & 0x100)
    characterize.base_qualities(prefix, aligned, characterize.quals_from_sam(prefix + ".sam")[1], eng)
    model.load_model(prefix, fastq=True)
    with pytest.raises(FileNotFoundError):
        model.load_model(prefix, chimeric=True, fastq=True)
    os.rename(prefix + "_chimeric_info.aside", prefix + "_chimeric_info")
    m = model.load_model(prefix, chimeric=True, fastq=True)
    gaps = np.array(fx["genome"]["gap_length"], dtype=np.int64)
    assert m.segment_mean == (len(gaps) + fx["n_reads"]) / fx["n_reads"] == 1.28 and m.abun_inflation is None
    assert np.array_equal(np.sort(m.kde[model.NS_KDE_GAP][0]), np.sort(np.log10(gaps + 1))) and m.kde[model.NS_KDE_GAP][1] == 0.01
    assert m.strandness_rate == round(fx["genome"]["strandness"], 3)
    e = EN.Engine(0)
    try:
        e.set_reference(small_ref)
        e.load_model(m)
        p = EN.make_params(seed=SEED, first_read=0, n_reads=3000, kind=EN.NS_KIND_ALIGNED, fastq=True, chimeric=True, max_len=small_ref.max_chrom)
        b = e.generate(p)
        got, reads, pieces = b.records().tobytes(), b.reads(), b.pieces()
    finally:
        e.close()
    exp = oracle_lib.generate(m, small_ref, p)
    assert got == exp["records"].tobytes() and len(got) > 3000 * 100
    assert np.array_equal(reads["seq_len"], exp["reads"]["seq_len"]) and len(reads) == 3000
    assert len(pieces) > 3000                                # chimeric reads among them: segment_mean is 1.28
