"""Training side, the read-length models ("Read lengths: the KDE inputs") on CPU: the engine's CIGAR walk and segment rule
(nanosim_amd/csrc/ns_read_len.h, compiled for the host; on the GPU k_len_scan, k_len_flag and k_len_reduce of ns_train.h run them) and
the host module around the call — pinned against what the REAL src/head_align_tail_dist.py and src/get_primary_sam.py collected for the
same records (tests/golden/reference_read_len.json.gz, tests/golden/make_read_len_golden.py) and against hand-made records."""
import ctypes as C
import gzip
import json
import os
import subprocess
import types

import numpy as np
import pytest

from nanosim_amd import characterize, engine, model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_KEYS = ("aligned_ref_length", "total_length", "ht_length", "head", "tail")


def load_fixture():
    with gzip.open(os.path.join(ROOT, "tests", "golden", "reference_read_len.json.gz"), "rt") as f:
        fx = json.load(f)
    fx["refs"] = [tuple(r) for r in fx["refs"]]
    fx["primary"] = [tuple(r) for r in fx["primary"]]
    t = fx["trx"]
    t["refs"], t["records"], t["genome_records"] = [tuple(r) for r in t["refs"]], [tuple(r) for r in t["records"]], [tuple(r) for r in t["genome_records"]]
    return fx


@pytest.fixture(scope="module")
def fx():
    return load_fixture()


def build_host_walk():
    """an object that stands in for an Engine: its ns_read_lengths is the engine's walk compiled for the host (tests/read_len_host.cpp)"""
    out = os.path.join(ROOT, "tests", "_tmp")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libread_len_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tests", "read_len_host.cpp")])
    L = C.CDLL(so)
    L.len_host_read_lengths.restype = C.c_int
    L.len_host_read_lengths.argtypes = [C.c_void_p] + [C.c_void_p] * 6 + [C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]

    def check(rc):
        if rc:
            raise engine.EngineError("host walk: error %d" % rc)
    return types.SimpleNamespace(ctx=None, _check=check, L=types.SimpleNamespace(ns_read_lengths=L.len_host_read_lengths))


@pytest.fixture(scope="module")
def host():
    return build_host_walk()


def check_figures(got: dict, exp: dict, transcriptome: bool = False):
    """every integer list and the ratio list of the reference, exactly"""
    for k in INT_KEYS + (("total_ref_length",) if transcriptome else ()):
        assert got[k].dtype == np.int64 and got[k].tolist() == exp[k], k
    assert got["head_vs_ht_ratio"].dtype == np.float64 and got["head_vs_ht_ratio"].tolist() == exp["head_vs_ht_ratio"]
    assert ("total_ref_length" in got) == transcriptome
    assert int(got["n_segments"].sum()) == len(exp["aligned_ref_length"]) and len(got["aln"]) >= len(got["n_segments"])


def check_genome(eng, fx):
    got = characterize.count_read_lengths(eng, fx["refs"], fx["primary"])
    check_figures(got, fx["genome"])
    return got


def check_transcriptome(eng, fx):
    t = fx["trx"]
    got = characterize.count_read_lengths(eng, t["refs"], t["records"], "transcriptome", t["genome_records"])
    check_figures(got, t, True)
    assert (got["n_segments"] == np.diff([i for i in range(len(t["records"])) if i == 0 or t["records"][i][0] != t["records"][i - 1][0]] + [len(t["records"])])).all()
    return got


def test_host_walk_reproduces_the_reference_in_genome_mode(fx, host):
    assert len(fx["primary"]) == 599 and len(fx["genome"]["total_length"]) == 405 and len(fx["genome"]["aligned_ref_length"]) == 558
    got = check_genome(host, fx)
    names = [r[0] for r in fx["primary"]]
    assert [names.index(fx["tags"]["across_block"][0]) + i for i in range(3)] == [255, 256, 257]
    # the last_is_edge quirk, read by read: a merge against the previous record's edge would give one segment fewer
    reads = list(dict.fromkeys(names))
    for name, n_seg in zip(fx["tags"]["quirk"], (3, 2)):
        assert got["n_segments"][reads.index(name)] == n_seg
    for name in fx["tags"]["triple"] + fx["tags"]["circ_SE"] + fx["tags"]["circ_ES"]:
        assert got["n_segments"][reads.index(name)] == 1
    # what the KDE step never sees, from pysam's definitions: a record's sums
    a = got["aln"][names.index(fx["tags"]["ops_N"][0])]                    # 10S300M1200N250=2X40M5P3I90M
    assert (a["read_len"], a["ref_len"], a["query_aln_len"], a["head"], a["tail"]) == (10 + 300 + 250 + 2 + 40 + 3 + 90, 300 + 1200 + 250 + 2 + 40 + 90, 685, 10, 0)


def test_host_walk_reproduces_the_reference_in_transcriptome_mode(fx, host):
    got = check_transcriptome(host, fx)
    t = fx["trx"]
    reads = list(dict.fromkeys(r[0] for r in t["records"]))
    own = characterize.count_read_lengths(host, t["refs"], t["records"], "transcriptome")
    in_genome = set(r[0] for r in t["genome_records"])
    smaller = [i for i, n in enumerate(reads) if got["head"][i] < own["head"][i] or got["tail"][i] < own["tail"][i]]
    assert smaller and all(reads[i] in in_genome for i in smaller)
    assert any(n not in in_genome for n in reads) and all(got["head"][i] == own["head"][i] for i, n in enumerate(reads) if n not in in_genome)
    assert (got["head"] <= own["head"]).all() and (got["tail"] <= own["tail"]).all()


def test_heads_tails_and_reference_lengths_equal_the_sam_pairs_walk(host):
    """where sam_records accepts a record, head, tail and ref_len equal ns_sam_aln's for it (ns_sam_aln states the clips in CIGAR
    order; the head of get_head_tail is the tail clip on a reverse record)"""
    from tests.test_sam_pairs import build_host_walk as build_sam_host
    from tests.test_sam_pairs import load_fixture as load_sam_fixture
    recs = load_sam_fixture()["records"]
    packed = characterize.pairs_from_sam(build_sam_host(), recs)
    refs = [(n, 1 << 30) for n in dict.fromkeys(r[2] for r in recs)]
    rc, out, got, _, _ = raw_call(host, refs, [r[:5] for r in recs])
    assert rc == 0 and len(got) == len(recs) == 341 and any(r[1] & 16 for r in recs) and packed.aln["head"].any() and packed.aln["tail"].any()
    # the records without a reference base (all insertion) are lines for the homopolymer model and bad records here: ns_read_len.h says why
    ok = packed.aln["ref_len"] != 0
    assert out.n_bad == int((~ok).sum()) > 0 and out.first_bad == int(np.argmin(ok)) and not got.view(np.uint32).reshape(-1, 6)[~ok].any()
    rev = np.array([bool(r[1] & 16) for r in recs])
    assert np.array_equal(got["head"][ok], np.where(rev, packed.aln["tail"], packed.aln["head"])[ok])
    assert np.array_equal(got["tail"][ok], np.where(rev, packed.aln["head"], packed.aln["tail"])[ok])
    assert np.array_equal(got["ref_len"], packed.aln["ref_len"]) and np.array_equal(got["query_aln_len"][ok], packed.aln["query_len"][ok])


def raw_call(eng, refs, records, read_off=None, mode=0):
    """ns_read_lengths without the ValueError of the module: (rc, the struct, aln, reads, segments)"""
    n = len(records)
    if read_off is None:
        read_off = np.arange(n + 1, dtype=np.uint64)
    read_off = np.ascontiguousarray(read_off, dtype=np.uint64)
    cg, cg_off = characterize._pack([r[4] for r in records])
    names = [r[0] for r in refs]
    ref_id = np.array([names.index(r[2]) for r in records], dtype=np.uint32)
    start = np.array([r[3] - 1 for r in records], dtype=np.uint64)
    reverse = np.array([1 if r[1] & 16 else 0 for r in records], dtype=np.uint8)
    total = np.array([r[1] for r in refs], dtype=np.uint64)
    aln = np.full(6 * n, 0xA5A5A5A5, dtype=np.uint32).view(characterize.LEN_ALN_DTYPE)
    reads = np.full(4 * (len(read_off) - 1), 0xA5A5A5A5, dtype=np.uint32).view(characterize.LEN_READ_DTYPE)
    seg = np.full(n, 0xA5A5A5A5, dtype=np.uint64)
    out = characterize.NsLenResult()
    out.aln, out.reads, out.segments = aln.ctypes.data if n else None, reads.ctypes.data if len(reads) else None, seg.ctypes.data if n else None
    rc = eng.L.ns_read_lengths(eng.ctx, cg.ctypes.data, cg_off.ctypes.data, reverse.ctypes.data, ref_id.ctypes.data, start.ctypes.data, total.ctypes.data,
                               len(refs), read_off.ctypes.data, len(read_off) - 1, n, mode, None, None, C.byref(out))
    return rc, out, aln, reads, seg


def rec(cigar, pos=1001, flag=0, name="r", rname="ref"):
    return (name, flag, rname, pos, cigar)


REF = [("ref", 10000)]
# every kind of bad record of ns_read_len.h
BAD = ("",                                      # empty
       "*", "10M5Z", "10M 5S", "10m", "5S-3M",  # a byte that is neither a digit nor an op
       "M10", "10MM", "5S10MS",                 # an op without a count
       "10M5",                                  # a count without an op
       "4294967295S1M", "4000000000M294967296D", "99999999999999999999M", "2147483648I2147483648=",      # a sum beyond 32 bits
       "10S5I", "7H", "3P")                     # no reference base
GOOD = ("1M", "0S1M", "4294967295M", "4294967294S1M", "5H10S3=2X1D7N4I2P9M1S2H")


def check_bad_records(eng):
    """each bad record alone, then all of them between good ones: the count and the smallest index"""
    for c in BAD:
        rc, out, aln, _, _ = raw_call(eng, REF, [rec(c)])
        assert rc == 0 and (out.n_bad, out.first_bad) == (1, 0), c
        assert not aln.view(np.uint32).any(), c
    for c in GOOD:
        rc, out, aln, _, _ = raw_call(eng, REF, [rec(c)])
        assert rc == 0 and (out.n_bad, out.first_bad) == (0, 1), c
    recs = [rec(GOOD[i % len(GOOD)]) for i in range(70)] + [rec(c) for c in BAD] + [rec("12M")] * 3
    rc, out, aln, _, _ = raw_call(eng, REF, recs)
    assert rc == 0 and (out.n_bad, out.first_bad) == (len(BAD), 70)
    assert aln["ref_len"][:70].all() and not aln.view(np.uint32).reshape(-1, 6)[70:70 + len(BAD)].any() and aln["ref_len"][-3:].tolist() == [12] * 3
    with pytest.raises(ValueError, match=r"%d SAM record\(s\).*first is record 70 \(r\)" % len(BAD)):
        characterize.count_read_lengths(eng, REF, recs)
    # a count without an op directly in front of a CIGAR that begins with an op letter (the CIGARs of a call lie one behind the other)
    recs = [rec("7M"), rec("10M5"), rec("M3M"), rec("12"), rec("S5M"), rec("9M")]
    rc, out, aln, _, _ = raw_call(eng, REF, recs)
    assert rc == 0 and (out.n_bad, out.first_bad) == (4, 1) and aln["ref_len"].tolist() == [7, 0, 0, 0, 0, 9] and aln["read_len"].tolist() == [7, 0, 0, 0, 0, 9]
    a = raw_call(eng, REF, [rec(GOOD[-1])])[2][0]
    assert (a["head"], a["tail"], a["read_len"], a["ref_len"], a["query_aln_len"]) == (5, 2, 5 + 10 + 3 + 2 + 4 + 9 + 1 + 2, 3 + 2 + 1 + 7 + 9, 3 + 2 + 4 + 9)


def test_bad_records_are_counted_with_the_first_index(host):
    check_bad_records(host)


def check_hand_cases(eng):
    """get_head_tail and edge_checker at their corners"""
    cases = [  # (cigar, flag, pos, LN) -> (head, tail, edge)
        (("5H10S100M", 0, 5000, 10000), (5, 0, 0)), (("5H10S100M", 16, 5000, 10000), (0, 5, 0)),
        (("3S100M9S", 16, 5000, 10000), (9, 3, 0)), (("100M4S6H", 0, 5000, 10000), (0, 6, 0)), (("8S", 0, 5000, 10000), (0, 0, 0)),
        (("100M", 0, 401, 10000), (0, 0, 1)), (("100M", 0, 402, 10000), (0, 0, 0)), (("99M", 0, 1, 10000), (0, 0, 0)),
        (("100M", 0, 9500, 10000), (0, 0, 2)), (("100M", 0, 9499, 10000), (0, 0, 0)),            # rend = 9599 = LN - 401 ; 9598
        (("99M", 0, 9900, 10000), (0, 0, 0)), (("150M", 0, 101, 600), (0, 0, 2)),                # start and end: the `elif` leaves the end
        (("100M", 0, 1, 300), (0, 0, 2)), (("50M50N", 0, 401, 10000), (0, 0, 1)), (("50M49D", 0, 401, 10000), (0, 0, 0))]
    for (cigar, flag, pos, total), exp in cases:
        rc, out, aln, reads, seg = raw_call(eng, [("ref", total)], [rec(cigar, pos, flag)])
        assert rc == 0
        if cigar == "8S":
            assert out.n_bad == 1
            continue
        assert out.n_bad == 0 and (int(aln[0]["head"]), int(aln[0]["tail"]), int(aln[0]["edge"])) == exp, (cigar, flag, pos, total)
        assert out.n_segments == 1 and seg[0] == aln[0]["ref_len"] and seg[0] != 0xA5A5A5A5 and reads[0].tolist() == (aln[0]["read_len"], exp[0], exp[1], 1)
    # one read of four records: start, end (joined), end on another reference, start (same reference as the record in front, first edge start: not joined)
    two = [("ref", 10000), ("other", 10000)]
    recs = [rec("200M5S", 1), rec("7S300M", 9700), rec("2S150M1S", 9800, rname="other"), rec("120M", 1, rname="other")]
    rc, out, aln, reads, seg = raw_call(eng, two, recs, [0, 4])
    assert rc == 0 and out.n_segments == 3 and seg[:3].tolist() == [500, 150, 120] and seg[3] == 0xA5A5A5A5
    assert reads[0].tolist() == (307, 0, 0, 3)
    rc, out, aln, reads, seg = raw_call(eng, two, recs, [0, 4], mode=1)
    assert rc == 0 and out.n_segments == 4 and seg.tolist() == [200, 300, 150, 120] and reads[0].tolist() == (307, 0, 0, 4)
    rc, out, aln, reads, seg = raw_call(eng, two, recs, [0, 1, 4])
    # (read off at record 1, the first edge is an end: the start on the other reference is joined to the end in front of it)
    assert rc == 0 and seg[:int(out.n_segments)].tolist() == [200, 300, 270] and [r.tolist() for r in reads] == [(205, 0, 5, 1), (307, 0, 0, 2)]


def test_hand_cases_of_clips_edges_and_segments(host):
    check_hand_cases(host)


def check_argument_errors(eng, einval=-1):
    recs = [rec("10M"), rec("20M")]
    for read_off in ([0, 1], [0, 2, 2], [1, 2], [0, 2, 1], [0, 1, 3]):
        assert raw_call(eng, REF, recs, read_off)[0] == einval, read_off
    assert raw_call(eng, REF, recs, mode=2)[0] == einval
    rc, out, aln, reads, seg = raw_call(eng, REF, [], [0])
    assert rc == 0 and (out.n_segments, out.n_bad, out.first_bad) == (0, 0, 0)


def test_argument_checks_of_the_host_shim(host):
    check_argument_errors(host)


def test_kde_models_equal_what_the_reference_fits(fx, host):
    got = characterize.count_read_lengths(host, fx["refs"], fx["primary"])
    m = characterize.kde_models(got, np.array(fx["unaligned_len"]))
    assert list(m) == ["aligned_region", "aligned_reads", "ht_length", "ht_ratio", "unaligned_length"]
    g = fx["genome"]
    exp = {"aligned_region": (np.array(g["aligned_ref_length"], dtype=np.float64), 10), "aligned_reads": (np.array(g["total_length"], dtype=np.float64), 10),
           "ht_length": (np.log10(np.array(g["ht_length"]) + 1), 0.01), "ht_ratio": (np.array(g["head_vs_ht_ratio"]), 0.01),
           "unaligned_length": (np.array(fx["unaligned_len"], dtype=np.float64), 10)}
    for name, (data, bw) in exp.items():
        assert m[name][0].dtype == np.float64 and np.array_equal(m[name][0], data) and m[name][1] == bw, name
    assert 0 in fx["unaligned_len"] and "unaligned_length" not in characterize.kde_models(got, np.array([], dtype=np.int64))
    assert "unaligned_length" not in characterize.kde_models(got)
    t = fx["trx"]
    got = characterize.count_read_lengths(host, t["refs"], t["records"], "transcriptome", t["genome_records"])
    m = characterize.kde_models(got)
    assert np.array_equal(m["aligned_region_2d"][0], np.array(t["rows_2d"], dtype=np.float64)) and m["aligned_region_2d"][1] == t["bw_2d"]
    assert np.array_equal(m["ht_length"][0], np.log10(np.array(t["ht_length"]) + 1))


def check_models_load_back(prefix, models):
    """<prefix>_kde.npz through model._load_kde / _load_kde2d"""
    npz = np.load(prefix + "_kde.npz")
    for name, (data, bw) in models.items():
        if name == "aligned_region_2d":
            x, y, b = model._load_kde2d(prefix, npz)
            order = np.argsort(data[:, 0], kind="stable")
            assert np.array_equal(x, data[order, 0]) and np.array_equal(y, data[order, 1]) and b == bw
        else:
            d, b = model._load_kde(prefix, name, npz)
            assert d.dtype == np.float64 and np.array_equal(d, data) and b == bw, name


def test_npz_and_pickles_load_back_exactly(fx, host, tmp_path):
    t = fx["trx"]
    got = characterize.count_read_lengths(host, t["refs"], t["records"], "transcriptome", t["genome_records"])
    models = characterize.kde_models(got, np.array(fx["unaligned_len"]))
    assert set(models) == set(characterize.KDE_NAMES)
    prefix = str(tmp_path / "npz_only")
    characterize.write_kde(prefix, models, pickles=False)
    assert sorted(os.listdir(str(tmp_path))) == ["npz_only_kde.npz"]
    check_models_load_back(prefix, models)
    prefix = str(tmp_path / "both")
    try:
        import joblib  # noqa: F401
        import sklearn.neighbors  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError):                    # scikit-learn is optional: asking for the pickles without it is an error
            characterize.write_kde(prefix, models, pickles=True)
        characterize.write_kde(prefix, models)
        assert not os.path.exists(prefix + "_ht_ratio.pkl")
        return
    characterize.write_kde(prefix, models, pickles=True)
    for name, (data, bw) in models.items():
        d, b = model._kde_pickle(prefix + "_" + name + ".pkl")
        assert np.array_equal(d, data if data.ndim == 2 else data[:, None]) and b == bw, name
    os.remove(prefix + "_kde.npz")                          # the reference's layout alone: load_model's second route
    for name in ("aligned_region", "aligned_reads", "ht_length", "ht_ratio", "unaligned_length"):
        d, b = model._load_kde(prefix, name, None)
        assert np.array_equal(d, models[name][0]) and b == models[name][1]
    x, y, b = model._load_kde2d(prefix, None)
    assert sorted(zip(x.tolist(), y.tolist())) == sorted(map(tuple, models["aligned_region_2d"][0].tolist())) and b == models["aligned_region_2d"][1]


def test_read_lengths_writes_the_files_of_the_reference(fx, host, tmp_path):
    prefix = str(tmp_path / "training")
    sam = str(tmp_path / "training.sam")
    with open(sam, "w") as f:
        f.write(fx["sam"])
    refs, recs, unaligned_len, strandness = characterize.primary_and_unaligned(sam)
    assert refs == fx["refs"] and recs == fx["primary"] and unaligned_len.tolist() == fx["unaligned_len"] and strandness == fx["strandness"]
    figures = characterize.read_lengths(prefix, refs, recs, host, unaligned_len, strandness, pickles=False)
    check_figures(figures, fx["genome"])
    assert open(prefix + "_strandness_rate").read() == fx["texts"]["strandness"]
    assert open(prefix + "_reads_alignment_rate").read() == fx["texts"]["alignment_rate"]
    check_models_load_back(prefix, characterize.kde_models(figures, unaligned_len))
    assert not [n for n in os.listdir(str(tmp_path)) if n.endswith(".txt")]
    characterize.read_lengths(prefix, refs, recs, host, np.array([], dtype=np.int64), strandness, pickles=False)
    assert open(prefix + "_reads_alignment_rate").read() == fx["texts"]["alignment_rate_all_aligned"]
    assert "unaligned_length_data" not in np.load(prefix + "_kde.npz")
    # what load_model reads of the two texts
    assert float(fx["texts"]["strandness"].split("\t")[1]) == round(fx["strandness"], 3)
    assert characterize.format_alignment_rate(405, len(fx["unaligned_len"])) == fx["texts"]["alignment_rate"]


def test_length_records_and_primary_and_unaligned(fx, tmp_path):
    primary = str(tmp_path / "primary.sam")
    with open(primary, "w") as f:
        f.write("".join("@SQ\tSN:%s\tLN:%d\n" % r for r in fx["refs"]))
        for i, r in enumerate(fx["primary"]):
            f.write("%s\t%d\t%s\t%d\t60\t%s\t*\t0\t0\t*\t*\n" % r)
            if i == 4:
                f.write("nocigar\t0\tchrA_1\t5\t60\t*\t*\t0\t0\tACGT\t*\n")
    refs, recs = characterize.length_records(primary)
    assert refs == fx["refs"] and recs == fx["primary"]
    with open(primary, "a") as f:
        f.write("stray\t0\tchrZ\t5\t60\t10M\t*\t0\t0\t*\t*\n")
    with pytest.raises(ValueError, match="stray lies on chrZ"):
        characterize.length_records(primary)
    only = str(tmp_path / "unmapped.sam")
    with open(only, "w") as f:
        f.write("@SQ\tSN:chrA_1\tLN:60000\nu1\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\t*\nsec\t256\tchrA_1\t5\t0\t4M\t*\t0\t0\t*\t*\n")
    with pytest.raises(ValueError, match="no primary alignment"):
        characterize.primary_and_unaligned(only)
    flags = [int(line.split("\t")[1]) for line in fx["sam"].splitlines() if not line.startswith("@")]
    assert any(f & 256 for f in flags) and any(f & 2048 for f in flags) and flags.count(4) == len(fx["unaligned_len"])


@pytest.mark.parametrize("mode", ("genome", "transcriptome"))
def test_length_figures_maf_equal_the_reference(fx, tmp_path, mode):
    path = str(tmp_path / "x_besthit.maf")
    with open(path, "w") as f:
        f.write("##maf version=1\na score=5\n" + fx["maf"]["text"])
    got = characterize.length_figures_maf(path, mode)
    exp = fx["maf"][mode]
    for k in ("aligned_ref_length", "total_length", "ht_length") + (("total_ref_length",) if mode == "transcriptome" else ()):
        assert got[k].tolist() == exp[k], k
    assert got["head_vs_ht_ratio"].tolist() == exp["head_vs_ht_ratio"] and 0 in exp["ht_length"] and len(exp["head_vs_ht_ratio"]) < 40
    assert (got["head"] + got["tail"] == got["ht_length"]).all() and ("total_ref_length" in got) == (mode == "transcriptome")
    m = characterize.kde_models(got)
    if mode == "transcriptome":
        assert np.array_equal(m["aligned_region_2d"][0], np.array(exp["rows_2d"], dtype=np.float64)) and m["aligned_region_2d"][1] == exp["bw_2d"]
    with open(path, "a") as f:
        f.write("s chrA_1 0 5 + 60000 ACGTA\n")
    with pytest.raises(ValueError, match="without its partner"):
        characterize.length_figures_maf(path, mode)


def test_c_abi_layout_and_export():
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "nanosim_amd.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(ns_len_result), offsetof(ns_len_result, reads), offsetof(ns_len_result, segments),
         offsetof(ns_len_result, n_segments), offsetof(ns_len_result, n_bad), offsetof(ns_len_result, first_bad), offsetof(ns_len_result, ms_kernel));
  printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(ns_len_aln), offsetof(ns_len_aln, head), offsetof(ns_len_aln, tail), offsetof(ns_len_aln, read_len),
         offsetof(ns_len_aln, ref_len), offsetof(ns_len_aln, query_aln_len), offsetof(ns_len_aln, edge));
  printf("%zu %zu %zu %zu %zu %d %d\n", sizeof(ns_len_read), offsetof(ns_len_read, read_len), offsetof(ns_len_read, head), offsetof(ns_len_read, tail),
         offsetof(ns_len_read, n_segments), NS_LEN_GENOME, NS_LEN_TRANSCRIPTOME);
  return 0; }'''
    out = os.path.join(ROOT, "tests", "_tmp")
    os.makedirs(out, exist_ok=True)
    src, exe = os.path.join(out, "read_len_abi.c"), os.path.join(out, "read_len_abi")
    with open(src, "w") as f:
        f.write(prog)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
    a, b, c = subprocess.check_output([exe]).decode().strip().split("\n")
    R = characterize.NsLenResult
    assert [int(v) for v in a.split()] == [C.sizeof(R), R.reads.offset, R.segments.offset, R.n_segments.offset, R.n_bad.offset, R.first_bad.offset, R.ms_kernel.offset]
    A, D = characterize.LEN_ALN_DTYPE, characterize.LEN_READ_DTYPE
    assert [int(v) for v in b.split()] == [A.itemsize] + [A.fields[n][1] for n in ("head", "tail", "read_len", "ref_len", "query_aln_len", "edge")]
    assert [int(v) for v in c.split()] == [D.itemsize] + [D.fields[n][1] for n in ("read_len", "head", "tail", "n_segments")] + \
        [characterize.LEN_GENOME, characterize.LEN_TRANSCRIPTOME]
    assert "ns_read_lengths" in engine.EXPORTS
    with open(os.path.join(ROOT, "include", "nanosim_amd.h")) as f:
        assert "#define NS_ABI_VERSION 7u" in f.read()        # an added function, no ABI bump


def test_walk_runs_clean_under_the_sanitizers_as_a_program(fx, tmp_path):
    """tests/read_len_host.cpp with its own main under -fsanitize=address,undefined: the fixture, then every bad record, each CIGAR in a
    buffer of exactly its size"""
    exe = os.path.join(ROOT, "tests", "_tmp", "read_len_asan")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DREAD_LEN_MAIN", "-o", exe,
           os.path.join(ROOT, "tests", "read_len_host.cpp")]
    # (the sanitizer's runtime linked statically when the compiler has it: such a program starts whatever the environment loads in front of it)
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode != 0:
        subprocess.check_call(cmd)
    names = [r[0] for r in fx["refs"]]
    lines = ["%d" % len(names)] + ["%d" % r[1] for r in fx["refs"]]
    prev = None
    for r in fx["primary"]:
        lines.append("%d %d %d %d %s" % (r[0] != prev, bool(r[1] & 16), names.index(r[2]), r[3] - 1, r[4]))
        prev = r[0]
    for c in BAD:
        if " " not in c:
            lines.append("1 0 0 1000 %s" % (c or "-"))
    path = str(tmp_path / "records.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:]
    n_bad = len([c for c in BAD if " " not in c])
    out = r.stdout.split("\n")
    assert out[0] == "%d %d %d" % (558 + n_bad, n_bad, 599) and out[1] == "%d %d %d" % (599 + n_bad, n_bad, 599)
