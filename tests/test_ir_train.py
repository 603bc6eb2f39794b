"""Training side, the intron-retention model ("Intron retention: the Markov counts") on CPU: the engine's walk over a read's
blocks and its transcript's introns (nanosim_amd/csrc/ns_ir_train.h, compiled for the host; on the GPU k_ir_walk of ns_train.h runs it)
and the host module around the call — pinned against what the REAL src/model_intron_retention.py (intron_retention) counted and wrote
for the same annotation and SAM text (tests/golden/reference_ir_train.json.gz, tests/golden/make_ir_train_golden.py), per read and in
total, and against hand-made inputs with their expectations written out."""
import ctypes as C
import gzip
import json
import os
import subprocess
import types

import numpy as np
import pytest

from nanosim_amd import characterize, engine, intron_retention as IR, model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = characterize.IR_NONE
BAD_CIGARS = ("", "10", "M", "10Q", "10M5", "M10", "10MM", "*", "10M 5M", "4294967296M", "4294967295M1D", "2147483648N2147483648M")


def load_fixture():
    with gzip.open(os.path.join(ROOT, "tests", "golden", "reference_ir_train.json.gz"), "rt") as f:
        return json.load(f)


@pytest.fixture(scope="module")
def fx():
    return load_fixture()


def build_host_walk():
    """an object that stands in for an Engine: its ns_ir_train is the engine's walk compiled for the host (tests/ir_train_host.cpp)"""
    out = os.path.join(ROOT, "tests", "_tmp")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libir_train_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tests", "ir_train_host.cpp")])
    L = C.CDLL(so)
    L.ir_host_train.restype = C.c_int
    L.ir_host_train.argtypes = [C.c_void_p] + [C.c_void_p] * 5 + [C.c_uint32, C.c_void_p, C.c_void_p]

    def check(rc):
        if rc:
            raise engine.EngineError("host walk: error %d" % rc)
    return types.SimpleNamespace(ctx=None, _check=check, L=types.SimpleNamespace(ns_ir_train=L.ir_host_train))


@pytest.fixture(scope="module")
def host():
    return build_host_walk()


def write_inputs(fx, tmp_path, case=None):
    """-> (gff, g_sam, t_sam) paths of the fixture's input, or of one of its small cases"""
    src = fx if case is None else fx["small"][case]
    paths = []
    for name, text in (("annotation.gff3", fx["gff"]), ("g.sam", src["g_sam"]), ("t.sam", src["t_sam"])):
        paths.append(os.path.join(str(tmp_path), name))
        with open(paths[-1], "w") as f:
            f.write(text)
    return paths


def expected_state(p):
    return 2 if p["retained"] else (1 if sum(p["counts"]) else 0)


def check_fixture(eng, fx, tmp_path, per_read=True):
    """everything the reference counted for the fixture's input, in total and per read, exactly; -> (introns, reads, counts)"""
    gff, g_sam, t_sam = write_inputs(fx, tmp_path)
    introns = characterize.ir_introns(gff)
    reads = characterize.ir_alignments(g_sam, t_sam)
    assert [r.qname for r in reads] == fx["order"] == [p["qname"] for p in fx["per_read"]]
    got = characterize.count_intron_retention(eng, introns, reads)
    assert got["first"] == fx["first"] and got["states"] == fx["states"]
    assert [[k, [list(x) for x in v]] for k, v in got["ir_info"].items()] == fx["ir_info"]
    assert got["state"].dtype == np.uint8 and got["state"].tolist() == [expected_state(p) for p in fx["per_read"]]
    assert characterize.format_ir_markov_model(got) == fx["markov_model"] and characterize.format_ir_info(got["ir_info"]) == fx["ir_info_text"]
    if per_read:
        for r, p in zip(reads, fx["per_read"]):
            one = characterize.count_intron_retention(eng, introns, [r])
            kept = [list(x) for v in one["ir_info"].values() for x in v]
            assert one["first"] + one["states"] == p["counts"] and kept == p["retained"] and one["state"].tolist() == [expected_state(p)], p
    return introns, reads, got


def test_host_walk_reproduces_the_reference(fx, host, tmp_path):
    assert len(fx["order"]) == 290 and fx["first"] == [256, 31] and fx["states"] == [1461, 81, 62, 36] and len(fx["ir_info"]) == 11
    introns, reads, got = check_fixture(host, fx, tmp_path)
    by = dict(zip(fx["order"], got["state"].tolist()))
    t = fx["tags"]
    assert all(by[t[k]] == 2 for k in ("across_D", "across_N", "across_I", "partial_equals_other", "boundary_of_next", "boundary_of_previous", "overlapping_pair",
                                       "other_chromosome", "word_border", "secondary_in_front", "dup_transcriptome"))
    assert all(by[t[k]] == 1 for k in ("pending_at_end", "partial_equals_none", "touching_pair", "no_intron_chromosome", "dup_genome", "supplementary_replaces"))
    assert all(by[t[k]] == 0 for k in ("transcript_without_introns", "transcript_absent", "transcript_rows_skipped"))
    assert t["genome_only"] not in by and t["transcriptome_only"] not in by
    # the annotation as the reference reads it: a transcript without intron rows has an entry, rows that do not resolve have none
    assert introns["TX5"] == [] and "TXskipped" not in introns and "TX6" not in introns
    assert introns["TX3"][0] == ("MT", 100, 200) and introns["ENST00000001"][0] == ("1", 1000, 1200) and introns["TX9"] == [("1", 50000, 50100), ("2", 50000, 50150)]
    assert [i[1] for i in introns["TX12"]] == [30500, 30100, 30900]                         # file order
    tables = characterize.ir_tables(introns)
    assert list(tables["chrom_id"]) == ["1", "2", "MT"] and "TX5" not in tables["trx_id"] and len(tables["trx_id"]) == 11
    k = tables["trx_id"]["ENST00000002"]
    a, b = int(tables["merged_off"][k]), int(tables["merged_off"][k + 1])
    assert list(zip(tables["merged_start"][a:b].tolist(), tables["merged_end"][a:b].tolist())) == [(5000, 5500), (7000, 7500)]
    k = tables["trx_id"]["TX3"]
    a, b = int(tables["merged_off"][k]), int(tables["merged_off"][k + 1])
    assert list(zip(tables["merged_start"][a:b].tolist(), tables["merged_end"][a:b].tolist())) == [(100, 260), (400, 470)]      # touching introns are one


@pytest.mark.parametrize("case", ["start_row_0", "no_ir_row_0", "ir_row_0", "both_state_rows_0"])
def test_files_equal_the_reference(fx, host, tmp_path, case):
    check_files(host, fx, tmp_path, case)


def check_files(eng, fx, tmp_path, case):
    gff, g_sam, t_sam = write_inputs(fx, tmp_path, case)
    prefix = os.path.join(str(tmp_path), "training")
    got = characterize.intron_retention(prefix, gff, g_sam, t_sam, eng)
    exp = fx["small"][case]
    assert got["first"] == exp["first"] and got["states"] == exp["states"]
    with open(prefix + "_IR_markov_model") as f:
        assert f.read() == exp["markov_model"]
    with open(prefix + "_IR_info") as f:
        assert f.read() == exp["ir_info_text"]


def test_whole_files_and_the_simulators_loader(fx, host, tmp_path):
    gff, g_sam, t_sam = write_inputs(fx, tmp_path)
    prefix = os.path.join(str(tmp_path), "training")
    characterize.intron_retention(prefix, gff, g_sam, t_sam, host)
    with open(prefix + "_IR_markov_model") as f:
        text = f.read()
    assert text == fx["markov_model"] == "succedent\tno_IR\tIR\nstart\t0.892\t0.108\nno_IR\t0.9475\t0.0525\nIR\t0.6327\t0.3673\n"
    with open(prefix + "_IR_info") as f:
        assert f.read() == fx["ir_info_text"]
    # the simulator's loader opens the prefix: the model written here, an annotation with introns added here, a genome, the transcripts
    ann = os.path.join(str(tmp_path), "ann.gff3")
    with open(ann, "w") as f:
        f.write("1\tx\texon\t1\t4\t.\t+\t.\tParent=transcript:T1\n1\tx\texon\t9\t14\t.\t+\t.\tParent=transcript:T1\n")
    assert characterize.add_introns(ann, prefix + "_added_intron_final.gff3") == 1
    fa = os.path.join(str(tmp_path), "g.fa")
    with open(fa, "w") as f:
        f.write(">1\n" + "ACGT" * 10 + "\n")
    tr = M.Reference(["T1"], np.frombuffer(b"ACGTACGTAC", dtype=np.uint8).copy(), np.array([0, 10], dtype=np.uint64), np.zeros(1, dtype=np.uint8))
    ir = IR.load(prefix, fa, tr)
    assert ir.p_no_ir == [0.892, 0.9475, 0.6327] and ir.p_ir == [0.108, 0.0525, 0.3673]
    assert list(ir.item_type) == [0, 1, 0] and list(ir.item_start) == [0, 4, 8] and list(ir.item_len) == [4, 4, 6] and list(ir.eligible) == [True]


def test_texts():
    f = characterize.format_ir_markov_model
    assert f(dict(first=[0, 0], states=[0, 0, 0, 0])) == "succedent\tno_IR\tIR\nstart\t0.0\t0.0\nno_IR\t0.0\t0.0\nIR\t0.0\t0.0\n"
    assert f(dict(first=[1, 2], states=[0, 0, 7, 0])) == "succedent\tno_IR\tIR\nstart\t0.3333\t0.6667\nno_IR\t0.0\t0.0\nIR\t1.0\t0.0\n"
    assert characterize.format_ir_info({"b": [(5, 9), (20, 30)], "a": [(1, 2)], "c": []}) == "trx_name\tintron_spos\tintron_epos\nb\t5,20\t9,30\na\t1\t2\n"


# ---- hand-made inputs: one transcript of two introns, [100, 150) and [300, 350), on chromosome 0; a second of 33 introns on chromosome 1 ------
def hand_tables():
    return characterize.ir_tables({"A": [("c0", 100, 150), ("c0", 300, 350)], "B": [("c1", 1000 + 100 * i, 1000 + 100 * i + 10 + i) for i in range(33)]})


def call(eng, reads, tables=None):
    """reads = [(cigar, start, chrom id, trx id)] -> (first + states, states per read, retained intron indices, n_bad, first_bad)"""
    tables = tables or hand_tables()
    out, state, bits = characterize.ir_train_call(eng, tables, [r[0] for r in reads], [r[1] for r in reads], [r[2] for r in reads], [r[3] for r in reads])
    return [int(v) for v in out.first] + [int(v) for v in out.states], state.tolist(), np.flatnonzero(bits).tolist(), int(out.n_bad), int(out.first_bad)


HAND = [
    ("read through the first", ("200M", 50, 0, 0), [0, 1, 0, 0, 1, 0], 2, [0]),
    ("read through both", ("400M", 50, 0, 0), [0, 1, 0, 0, 0, 1], 2, [0, 1]),
    ("the second alone", ("200M", 250, 0, 0), [1, 0, 0, 1, 0, 0], 2, [1]),
    ("spliced", ("50M50N150M50N20M", 50, 0, 0), [1, 0, 1, 0, 0, 0], 1, []),
    ("the run ends with the read: dropped", ("100M", 50, 0, 0), [1, 0, 1, 0, 0, 0], 1, []),
    ("... one base behind the intron: flushed", ("101M", 50, 0, 0), [0, 1, 0, 0, 1, 0], 2, [0]),
    ("a block that begins inside: 49 bases equal nothing", ("100M", 101, 0, 0), [1, 0, 1, 0, 0, 0], 1, []),
    ("a run of 25 + 25 over both introns, N between: as long as either", ("75M200N75M", 50, 0, 0), [0, 1, 0, 0, 0, 1], 2, [0, 1]),
    ("D inside the intron shortens the run", ("70M5D125M", 50, 0, 0), [1, 0, 1, 0, 0, 0], 1, []),
    ("I inside the intron does not", ("70M5I130M", 50, 0, 0), [0, 1, 0, 0, 1, 0], 2, [0]),
    ("= and X are blocks, S H P are nothing", ("3H4S50=2P50X7I100M9S", 50, 0, 0), [0, 1, 0, 0, 1, 0], 2, [0]),
    ("a block of 0 bases", ("0M200M0X", 50, 0, 0), [0, 1, 0, 0, 1, 0], 2, [0]),
    ("another chromosome: outside everywhere", ("400M", 50, 1, 0), [1, 0, 1, 0, 0, 0], 1, []),
    ("no chromosome id", ("400M", 50, NONE, 0), [1, 0, 1, 0, 0, 0], 1, []),
    ("no transcript id", ("400M", 50, 0, NONE), [0, 0, 0, 0, 0, 0], 0, []),
    ("intron 31 of 33: the last bit of the first word", ("100M", 4050, 1, 1), [1, 0, 30, 1, 1, 0], 2, [2 + 31]),
    ("intron 32: the second word", ("100M", 4150, 1, 1), [1, 0, 31, 1, 0, 0], 2, [2 + 32]),
    ("introns 30 .. 32", ("300M", 3950, 1, 1), [1, 0, 29, 1, 0, 2], 2, [2 + 30, 2 + 31, 2 + 32]),
    ("the largest coordinates", ("4294967295M", 0, 0, 0), [0, 1, 0, 0, 0, 1], 2, [0, 1]),
]


@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_hand_made_reads(host, case):
    check_hand(host, case)


def check_hand(eng, case):
    _, read, counts, state, retained = case
    assert call(eng, [read]) == (counts, [state], retained, 0, 1)


def test_reads_add_up_and_the_bitmap_is_a_union(host):
    check_union(host)


def check_union(eng):
    reads = [c[1] for c in HAND]
    counts, state, retained, n_bad, first_bad = call(eng, reads)
    assert counts == [sum(c[2][i] for c in HAND) for i in range(6)] and state == [c[3] for c in HAND]
    assert retained == sorted(set(i for c in HAND for i in c[4])) and (n_bad, first_bad) == (0, len(reads))


@pytest.mark.parametrize("bad", BAD_CIGARS, ids=[repr(b) for b in BAD_CIGARS])
def test_bad_cigars(host, bad):
    check_bad(host, bad)


def check_bad(eng, bad):
    """a bad read counts nothing and marks nothing, wherever it stands; first_bad is the smallest index"""
    good = ("200M", 50, 0, 0)
    counts, state, retained, n_bad, first_bad = call(eng, [good, (bad, 50, 0, 0), ("200M", 250, 0, 0), (bad, 50, 0, NONE)])
    assert (counts, state, retained, n_bad, first_bad) == ([1, 1, 0, 1, 1, 0], [2, 0, 2, 0], [0, 1], 2, 1)


def test_bad_cigar_corners(host):
    check_bad_corners(host)


def check_bad_corners(eng):
    # a run that has already marked its row when the CIGAR turns out bad leaves nothing behind
    assert call(eng, [("200M5Q", 50, 0, 0)]) == ([0] * 6, [0], [], 1, 0)
    # the reference position may reach 2^32 - 1 and no further, whatever moves it
    top = 2 ** 32 - 1
    assert call(eng, [("10M", top - 10, 0, 0)])[3] == 0 and call(eng, [("10M", top - 9, 0, 0)])[3] == 1
    assert call(eng, [("5M5D", top - 9, 0, 0)])[3] == 1 and call(eng, [("5M5N", top - 9, 0, 0)])[3] == 1 and call(eng, [("5M5I5S", top - 5, 0, 0)])[3] == 0
    # a count without an op directly in front of a CIGAR that begins with an op letter: both are bad, each on its own
    counts, state, _, n_bad, first_bad = call(eng, [("7M", 0, 0, 0), ("10", 0, 0, 0), ("M", 0, 0, 0), ("9M", 0, 0, 0)])
    assert (counts, state, n_bad, first_bad) == ([2, 0, 2, 0, 0, 0], [1, 0, 0, 1], 2, 1)
    # count_intron_retention names the first
    with pytest.raises(ValueError, match="read q2"):
        characterize.count_intron_retention(eng, {"A": [("c0", 100, 150)]}, [characterize.IrRead("q1", "c0", 5, "9M", "A"), characterize.IrRead("q2", "c0", 5, "*", "A")])
    with pytest.raises(ValueError, match="start"):
        characterize.count_intron_retention(eng, {"A": [("c0", 100, 150)]}, [characterize.IrRead("q1", "c0", -1, "9M", "A")])


def test_input_validation(host):
    check_validation(host, engine.EngineError)


def check_validation(eng, error):
    ok = [("200M", 50, 0, 0)]
    assert call(eng, [], hand_tables()) == ([0] * 6, [], [], 0, 0)                           # no read: valid, all zeros
    for what, change in (("intr_off", lambda t: t["intr_off"].__setitem__(0, 1)), ("intr_off", lambda t: t["intr_off"].__setitem__(1, 40)),
                         ("merged_off", lambda t: t["merged_off"].__setitem__(1, 40)), ("intr_chrom", lambda t: t["intr_chrom"].__setitem__(0, 2)),
                         ("intr_end", lambda t: t["intr_end"].__setitem__(0, 99)), ("merged_chrom", lambda t: t["merged_chrom"].__setitem__(1, 2)),
                         ("merged_end", lambda t: t["merged_end"].__setitem__(0, 100)), ("merged_start", lambda t: t["merged_start"].__setitem__(1, 150)),
                         ("merged_start", lambda t: t["merged_start"].__setitem__(1, 90))):
        t = hand_tables()
        change(t)
        with pytest.raises(error):
            call(eng, ok, t)
        with pytest.raises(error):
            call(eng, [], t)                                                                 # the tables are checked without reads too
    for read in (("200M", 50, 2, 0), ("200M", 50, 0, 2), ("200M", 50, NONE - 1, 0)):
        with pytest.raises(error):
            call(eng, ok + [read])
    # 2^31 introns or merged intervals are refused before any of them is looked at
    for name in ("intr_off", "merged_off"):
        t = hand_tables()
        t[name][1:] = 2 ** 31
        with pytest.raises(error):
            call(eng, ok, t)
    # a transcript without introns between two that have some, and an intron of no bases: both are valid tables
    t = hand_tables()
    t["trx_id"] = {"A": 0, "none": 1, "B": 2}
    t["intr_off"] = np.array([0, 2, 2, 35], dtype=np.uint64)
    t["merged_off"] = np.array([0, 2, 2, 35], dtype=np.uint64)
    assert call(eng, [("200M", 50, 0, 0), ("200M", 50, 0, 1), ("100M", 4150, 1, 2)], t) == ([1, 1, 31, 1, 1, 0], [2, 0, 2], [0, 2 + 32], 0, 3)
    t = characterize.ir_tables({"A": [("c0", 100, 100), ("c0", 300, 350), ("c0", 350, 350)]})
    assert t["merged_start"].tolist() == [300] and call(eng, [("200M", 250, 0, 0)], t) == ([1, 0, 0, 1, 0, 1], [2], [1, 2], 0, 1)
    # a transcript id of NONE with no table at all
    empty = characterize.ir_tables({"T": []})
    assert int(empty["intr_off"][-1]) == 0 and call(eng, [("200M", 50, NONE, NONE)], empty) == ([0] * 6, [0], [], 0, 1)
    with pytest.raises(ValueError):
        characterize.ir_tables({"A": [("c0", 150, 100)]})
    with pytest.raises(ValueError):
        characterize.ir_tables({"A": [("c0", 100, 2 ** 32)]})


def test_ir_alignments_joins(tmp_path):
    def sam(name, rows):
        path = os.path.join(str(tmp_path), name)
        with open(path, "w") as f:
            f.write("@HD\tVN:1.6\n" + "".join("%s\t%d\t%s\t%d\t60\t%s\t*\t0\t0\t*\t*\n" % r for r in rows))
        return path
    g = sam("g.sam", [("a", 0, "chr1", 101, "50M"), ("u", 4, "*", 0, "*"), ("b", 16, "chr2", 7, "5M"), ("a", 2048, "chrX", 9, "7M"), ("c", 256, "1", 1, "3M"),
                      ("b", 4, "*", 0, "*")])
    t = sam("t.sam", [("b", 0, "ENST01.7", 1, "5M"), ("a", 0, "ENSG01.7", 1, "5M"), ("d", 0, "T", 1, "5M"), ("b", 256, "TX.1", 1, "5M"), ("c", 4, "*", 0, "*")])
    assert characterize.ir_alignments(g, t) == [("a", "chrX", 8, "7M", "ENSG01.7"), ("b", "chr2", 6, "5M", "TX.1")]
    assert characterize.ir_alignments(g, sam("t2.sam", [("b", 0, "ENST01.7", 1, "5M")])) == [("b", "chr2", 6, "5M", "ENST01")]


def test_add_introns_round_trip(tmp_path):
    """a property, not a comparison with GenomeTools: through both readers of the file the introns are exactly the gaps between a
    transcript's exons, every row resolves to its transcript, and nothing else of the annotation moves"""
    rng = np.random.default_rng(7)
    rows, exons = ["##gff-version 3\n"], {}
    styles = ("transcript_id=%s.3;gene_id=G", "Parent=transcript:%s;Name=e", "ID=exon:9;Parent=transcript:%s", "Parent=%s,other")
    for k in range(12):
        tid, chrom, strand = "TR%02d" % k, ("chr1", "2", "chrM")[k % 3], "+-"[k % 2]
        pos, own = int(rng.integers(1, 500)), []
        for _ in range(int(rng.integers(1, 7))):
            ln = int(rng.integers(5, 200))
            own.append((pos, pos + ln - 1))
            pos += ln + int(rng.integers(0, 3)) * int(rng.integers(1, 300))              # a third of the exons touch the next one
        if k == 5:
            own.append((own[0][0] + 1, own[0][1] + 2))                                     # an exon that overlaps another
        exons[tid] = sorted(own)
        order = list(own)
        rng.shuffle(order)
        rows.append("%s\tsrc\tmRNA\t%d\t%d\t.\t%s\t.\tID=transcript:%s\n" % (chrom, own[0][0], pos, strand, tid))
        for j, (s, e) in enumerate(order):
            rows.append("%s\tsrc\texon\t%d\t%d\t.\t%s\t.\t%s\n" % (chrom, s, e, strand, styles[k % 4] % tid))
            if j == 0:
                rows.append("%s\tsrc\tCDS\t%d\t%d\t.\t%s\t0\tParent=transcript:%s\n" % (chrom, s, e, strand, tid))
    rows.append("chr1\tsrc\texon\t5\t9\t.\t+\t.\tID=orphan\n")
    src, out = os.path.join(str(tmp_path), "in.gff3"), os.path.join(str(tmp_path), "out.gff3")
    with open(src, "w") as f:
        f.write("".join(rows))
    n = characterize.add_introns(src, out)
    want = {}
    for tid, own in exons.items():
        gaps, reach = [], None
        for s, e in own:
            if reach is not None and s > reach + 1:
                gaps.append((reach, s - 1))                                                # 0-based half-open: [end of the exon, start - 1 of the next)
            reach = e if reach is None else max(reach, e)
        want[tid] = gaps
    assert n == sum(len(g) for g in want.values()) and n > 10
    structure = IR.read_structure(out)
    introns = characterize.ir_introns(out)
    assert set(structure) == set(exons) and set(exons) <= set(introns)
    for tid, own in exons.items():
        items = structure[tid]
        assert [(i[2], i[3]) for i in items if i[0] == "intron"] == want[tid] == [(i[1], i[2]) for i in introns[tid]]
        assert [(i[2] + 1, i[3]) for i in items if i[0] == "exon"] == own                  # every exon, sorted by start
        assert [i[2] for i in items] == sorted(i[2] for i in items) and len(set((i[1], i[5]) for i in items)) == 1
    with open(out) as f:
        lines = f.readlines()
    kept = [l for l in rows if "\texon\t" not in l or "ID=orphan" in l]
    assert [l for l in lines if "\texon\t" not in l and "\tintron\t" not in l or "ID=orphan" in l] == kept
    assert characterize.add_introns(out, src) == n                                         # a second pass writes the same introns anew ...
    assert IR.read_structure(src) == structure                                             # ... in place of those that were there


def test_struct_layouts_and_exports(tmp_path):
    src = os.path.join(str(tmp_path), "layout.c")
    with open(src, "w") as f:
        f.write('''#include <stdio.h>
#include <stddef.h>
#include "nanosim_amd.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(ns_ir_train_result), offsetof(ns_ir_train_result, state), offsetof(ns_ir_train_result, retained),
         offsetof(ns_ir_train_result, first), offsetof(ns_ir_train_result, states), offsetof(ns_ir_train_result, n_bad), offsetof(ns_ir_train_result, first_bad),
         offsetof(ns_ir_train_result, ms_kernel));
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(ns_ir_introns), offsetof(ns_ir_introns, n_trx), offsetof(ns_ir_introns, n_chrom),
         offsetof(ns_ir_introns, intr_off), offsetof(ns_ir_introns, intr_chrom), offsetof(ns_ir_introns, intr_start), offsetof(ns_ir_introns, intr_end),
         offsetof(ns_ir_introns, merged_off), offsetof(ns_ir_introns, merged_chrom), offsetof(ns_ir_introns, merged_start), offsetof(ns_ir_introns, merged_end));
  printf("%u %d %d %d\\n", NS_IR_NONE, NS_IR_READ_NONE, NS_IR_READ_NO_IR, NS_IR_READ_IR);
  return 0;
}
''')
    exe = os.path.join(str(tmp_path), "layout")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
    rows = [[int(v) for v in l.split()] for l in subprocess.check_output([exe]).decode().splitlines()]
    for row, S in zip(rows, (characterize.NsIrTrainResult, characterize.NsIrIntrons)):
        assert row == [C.sizeof(S)] + [getattr(S, n).offset for n, _ in S._fields_]
    assert rows[2] == [NONE, characterize.IR_READ_NONE, characterize.IR_READ_NO_IR, characterize.IR_READ_IR]
    assert "ns_ir_train" in engine.EXPORTS
    with open(os.path.join(ROOT, "include", "nanosim_amd.h")) as f:
        assert "#define NS_ABI_VERSION 7u" in f.read()            # an added function, no ABI bump


def sanitizer_input(fx, tmp_path):
    """the fixture's tables and reads, the hand-made reads and one bad read as the text the stand-alone program takes; -> (path, n_reads)"""
    gff, g_sam, t_sam = write_inputs(fx, tmp_path)
    tables = characterize.ir_tables(characterize.ir_introns(gff))
    reads = characterize.ir_alignments(g_sam, t_sam)
    rows = ["%d %d" % (len(tables["trx_id"]), len(tables["chrom_id"]))]
    for k in range(len(tables["trx_id"])):
        a, b, c, d = (int(tables[n][k + i]) for n in ("intr_off", "merged_off") for i in (0, 1))
        rows.append("%d %d" % (b - a, d - c))
        rows += ["%d %d %d" % (tables["intr_chrom"][i], tables["intr_start"][i], tables["intr_end"][i]) for i in range(a, b)]
        rows += ["%d %d %d" % (tables["merged_chrom"][i], tables["merged_start"][i], tables["merged_end"][i]) for i in range(c, d)]
    for r in reads:
        rows.append("%d %d %d %s" % (r.start, tables["chrom_id"].get(characterize._strip_chr(r.chrom), -1), tables["trx_id"].get(r.trx, -1), r.cigar))
    rows.append("5 0 0 -")                                     # an empty CIGAR: bad
    rows.append("%d 0 0 10M" % (2 ** 32 - 5))                  # beyond the last coordinate: bad
    path = os.path.join(str(tmp_path), "reads.txt")
    with open(path, "w") as f:
        f.write("\n".join(rows) + "\n")
    return path, len(reads) + 2


def test_host_walk_is_clean_under_the_sanitizers(fx, tmp_path):
    """the walk as a stand-alone program with -fsanitize=address,undefined on the fixture's reads: exact-size buffers, so a byte read
    past a CIGAR, an element past a table or a word past a row is an error"""
    path, n_reads = sanitizer_input(fx, tmp_path)
    exe = os.path.join(str(tmp_path), "ir_train_host_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DIR_TRAIN_MAIN", "-o", exe,
                           os.path.join(ROOT, "tests", "ir_train_host.cpp")])
    out = subprocess.run([exe, path], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    assert [int(v) for v in out.stdout.splitlines()[0].split()] == fx["first"] + fx["states"] + [2, n_reads - 2]
