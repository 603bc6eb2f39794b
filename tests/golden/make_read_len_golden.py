#!/usr/bin/env python3
"""Golden fixture of the training side's read-length models ("Read lengths: the KDE inputs"): the REAL reference's
src/head_align_tail_dist.py (head_align_tail, A:58-281) and the non-chimeric primary_and_unaligned of src/get_primary_sam.py
(G:145-217) are run in the build container on synthetic alignments, and what they collect is committed as data.

Both read their alignments through pysam, which this image lacks, so the modules are imported unmodified with a pysam stand-in whose
AlignmentFile serves header['SQ'], fetch, query_name, reference_name, cigartuples, is_reverse, reference_start, reference_end,
reference_length, query_alignment_length, infer_read_length, query_length, flag and the is_* bits, and takes write().  joblib.dump and
KernelDensity are replaced by recorders: the arrays handed to fit() are the fixture.  The per-read heads and tails come from the
debugging files the reference writes next to them (<prefix>_head.txt, _tail.txt, A:186, 190).  The two small texts
(_strandness_rate, _reads_alignment_rate) are written by lines 833-851 of src/read_analysis.py, executed as they stand.
log10 values are NOT stored: the script checks that the array handed to the ht_length KDE is np.log10(ht + 1) of the integers it
stores, and the tests compute that on the machine they run on.

The input: about 600 records in about 400 reads on three references of 5 000, 20 000 and 60 000 bases, plus unmapped, secondary and
supplementary records; and a transcriptome variant with a genome file.  Every branch named in main()'s asserts is present.

    python tests/golden/make_read_len_golden.py        -> tests/golden/reference_read_len.json.gz
"""
import gzip
import json
import os
import shutil
import sys
import tempfile
import textwrap
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF_SRC = "/root/reference/src"
REFS = [("chrA_1", 60000), ("chrB_1", 20000), ("chrC_1", 5000)]
LN = dict(REFS)
TRX_REFS = [("tx1", 800), ("tx2", 1500), ("tx3", 2400), ("tx4", 3100), ("tx5", 5000)]
OPS = "MIDNSHP=X"


def cigartuples(cigar):
    out, num = [], ""
    for c in cigar:
        if c.isdigit():
            num += c
        else:
            out.append((OPS.index(c), int(num)))
            num = ""
    assert not num and out
    return out


def sums(cigar):
    """(read_len, ref_len, query_aln_len) as pysam states them"""
    t = cigartuples(cigar)
    return (sum(n for o, n in t if OPS[o] in "MISH=X"), sum(n for o, n in t if OPS[o] in "MDN=X"), sum(n for o, n in t if OPS[o] in "MI=X"))


def edge_of(rec):
    """(start, end) of edge_checker, restated only for the asserts on the input"""
    start, ref_len, total = rec[3] - 1, sums(rec[4])[1], LN[rec[2]]
    if ref_len < 100:
        return (False, False)
    if start + ref_len >= total - 1 - 400:
        return (False, True)
    return (start <= 400, False)


class Maker:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.n = 0

    def body(self, ref_len, fancy=False):
        """ops that cover exactly ref_len reference bases"""
        r = self.rng
        if ref_len < 40:
            return "%dM" % ref_len
        a = int(r.integers(5, ref_len // 3))
        d = int(r.integers(1, 6))
        b = int(r.integers(5, ref_len // 3))
        c = ref_len - a - b - d
        if fancy:
            x = int(r.integers(1, 4))
            return "%d=%dX%dI%dM%dD%dM" % (a - x, x, int(r.integers(1, 9)), b, d, c)
        return "%dM%dI%dM%dD%dM" % (a, int(r.integers(1, 9)), b, d, c)

    def clips(self, kind=None):
        r = self.rng
        kind = int(r.integers(0, 8)) if kind is None else kind
        h, t = int(r.integers(1, 120)), int(r.integers(1, 120))
        return [("", ""), ("%dS" % h, ""), ("", "%dS" % t), ("%dS" % h, "%dS" % t), ("%dH" % h, ""), ("", "%dH" % t), ("%dH" % h, "%dH" % t),
                ("%dH%dS" % (h, t), "%dS%dH" % (t, h))][kind]

    def cigar(self, ref_len, kind=None, fancy=False):
        h, t = self.clips(kind)
        return h + self.body(ref_len, fancy) + t

    def name(self):
        self.n += 1
        return "read%04d" % self.n

    def at(self, where, rname, ref_len):
        total = LN[rname]
        r = self.rng
        if where == "S":
            return int(r.integers(0, 401)) + 1
        if where == "E":
            return total - ref_len - int(r.integers(0, 401)) + 1
        return int(r.integers(500, total - ref_len - 1000)) + 1

    def rec(self, name, where, rname, ref_len=None, flag=None, cigar=None, kind=None, fancy=False):
        if ref_len is None:
            ref_len = int(self.rng.integers(150, 1800))
        if cigar is None:
            cigar = self.cigar(ref_len, kind, fancy)
        if flag is None:
            flag = 16 if self.rng.random() < 0.5 else 0
        return (name, flag, rname, self.at(where, rname, ref_len), cigar)

    def read(self, *parts, **kw):
        name = self.name()
        return [self.rec(name, *p, **kw) if isinstance(p, tuple) else self.rec(name, **p) for p in parts]


def genome_input():
    """(reads: lists of primary records in file order, tags: {what: [read names]})"""
    m = Maker(20261019)
    tags = {}

    def tag(what, read):
        tags.setdefault(what, []).append(read[0][0])
        return read
    special = []
    for i in range(12):
        ref = REFS[i % 3][0]
        special.append(tag("circ_SE", m.read(("S", ref), ("E", ref))))
        special.append(tag("circ_ES", m.read(("E", ref), ("S", ref))))
    for i in range(6):
        ref = REFS[i % 2][0]
        special.append(tag("triple", m.read(("S", ref), ("E", ref), ("E", ref)) if i % 2 else m.read(("E", ref), ("S", ref), ("S", ref))))
    for i in range(3):
        special.append(tag("wrong_edge", m.read(("S", "chrA_1"), ("M", "chrA_1"))))
        special.append(tag("wrong_edge", m.read(("S", "chrB_1"), ("S", "chrB_1"))))
        special.append(tag("wrong_edge", m.read(("M", "chrA_1"), ("E", "chrA_1"))))
        special.append(tag("len99", m.read(("S", "chrB_1"), ("E", "chrB_1", 99))))
        special.append(tag("len99", m.read(("S", "chrC_1", 99), ("E", "chrC_1"))))
        special.append(tag("other_ref", m.read(("S", "chrA_1"), ("E", "chrB_1"))))
        special.append(tag("other_ref", m.read(("S", "chrA_1"), ("E", "chrB_1"), ("E", "chrA_1"))))
        special.append(tag("second_segment_grows", m.read(("S", "chrA_1"), ("S", "chrA_1"), ("E", "chrA_1"))))
    # the last_is_edge quirk: a record that would merge against the edge of the record in front of it, but not against the first record's
    special.append(tag("quirk", m.read(("M", "chrA_1"), ("S", "chrA_1"), ("E", "chrA_1"))))
    special.append(tag("quirk", m.read(("S", "chrB_1"), ("E", "chrB_1"), ("S", "chrB_1"))))
    # clips
    nm = m.name()
    special.append(tag("5H10S", [(nm, 0, "chrA_1", 7000, "5H10S" + m.body(700) + "3S8H")]))
    nm = m.name()
    special.append(tag("rev_unequal", [(nm, 16, "chrA_1", 9000, "11S" + m.body(500) + "47S")]))
    nm = m.name()
    special.append(tag("rev_unequal", [(nm, 16, "chrB_1", 3000, "7H" + m.body(400, fancy=True)), (nm, 16, "chrB_1", 9000, m.body(300) + "21H")]))
    for kind in range(8):
        special.append(tag("clip%d" % kind, m.read(dict(where="M", rname="chrA_1", kind=kind, flag=0, fancy=True))))
    nm = m.name()
    special.append(tag("ops_N", [(nm, 0, "chrA_1", 2000, "10S300M1200N250=2X40M5P3I90M")]))
    nm = m.name()
    special.append(tag("nine_digits", [(nm, 0, "chrA_1", 30000, "200M123456789N150M4S")]))
    nm = m.name()
    long_ops = "".join("%dM%d%s" % (1 + i % 3, 1 + i % 2, "ID"[i % 2]) for i in range(2600))
    special.append(tag("long", [(nm, 16, "chrA_1", 20000, "6S" + long_ops + "9M")]))
    assert len(cigartuples(special[-1][0][4])) >= 5000
    # the ratio's two conditions: an earlier read with head == 0 and ht != 0 (not taken, A:180), one with ht == 0
    nm = m.name()
    special.append(tag("head0_earlier", [(nm, 0, "chrB_1", 5000, m.body(600) + "25S")]))
    nm = m.name()
    special.append(tag("ht0", [(nm, 0, "chrB_1", 6000, m.body(600))]))
    m.rng.shuffle(special)
    across = tag("across_block", m.read(("S", "chrA_1"), ("E", "chrA_1"), ("M", "chrB_1")))
    nm = m.name()
    first = tag("first_single", [(nm, 0, "chrC_1", 1200, "13S" + m.body(900) + "2S")])
    nm = m.name()
    last = tag("last_single", [(nm, 0, "chrA_1", 41000, m.body(800) + "30S")])                    # head == 0, ht != 0: taken (A:219)

    def filler():
        ref = REFS[int(m.rng.integers(0, 3))][0]
        return m.read(("M", ref)) if m.rng.random() < 0.65 else m.read(("M", ref), ("M", REFS[int(m.rng.integers(0, 2))][0]))
    reads = [first]
    count = 1
    pending = list(special)
    while count < 255:                                           # the three records of `across` sit at indices 255 .. 257
        nxt = pending.pop() if pending and count + len(pending[-1]) <= 255 and m.rng.random() < 0.3 else filler()
        if count + len(nxt) > 255:
            nxt = m.read(("M", "chrA_1"))
        reads.append(nxt)
        count += len(nxt)
    assert count == 255
    reads.append(across)
    count += 3
    while pending or count < 598:
        nxt = pending.pop() if pending and (m.rng.random() < 0.3 or count >= 598) else filler()
        reads.append(nxt)
        count += len(nxt)
    reads.append(last)
    return reads, tags


def full_sam(reads, seed=5):
    """the whole SAM file as records (qname, flag, rname, pos, cigar, seq): the primary ones plus, in between, unmapped reads (some with
    `*` as SEQ), secondary and supplementary records"""
    rng = np.random.default_rng(seed)
    out = []
    k = 0
    for read in reads:
        for r in read:
            out.append(r + ("*",))
        u = rng.random()
        if u < 0.12:
            k += 1
            out.append(("unmapped%03d" % k, 4, "*", 0, "*", "*" if k % 7 == 3 else "ACGT" * int(rng.integers(1, 300)) + "A" * (k % 4)))
        elif u < 0.18:
            out.append((read[0][0], 256 | (16 if u < 0.15 else 0), "chrA_1", 777, "50S200M", "*"))
        elif u < 0.24:
            out.append((read[0][0], 2048, "chrB_1", 888, "200M50H", "*"))
    out.append(("unmapped_tail", 4, "*", 0, "*", "ACGTACGTAC"))
    return out


def sam_text(refs, records):
    head = "@HD\tVN:1.6\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs) + "@PG\tID:synthetic\n"
    return head + "".join("%s\t%d\t%s\t%d\t%d\t%s\t*\t0\t0\t%s\t*\n" % (q, f, r, p, 0 if f & 4 else 60, c, s) for q, f, r, p, c, s in records)


def install_standins(files, written):
    """pysam / joblib / sklearn.neighbors stand-ins; files: {path: (refs, records)}; written: {path: [alignments]}; -> the recorder"""
    class Aln:
        def __init__(self, rec):
            self.rec = rec
            self.query_name, self.flag, self.reference_name, pos, self.cigarstring, seq = rec
            self.cigartuples = None if self.cigarstring == "*" else cigartuples(self.cigarstring)
            self.is_unmapped, self.is_reverse = bool(self.flag & 4), bool(self.flag & 16)
            self.is_secondary, self.is_supplementary = bool(self.flag & 256), bool(self.flag & 2048)
            self.query_length = 0 if seq == "*" else len(seq)
            self.reference_start = pos - 1
            self.reference_length = self.reference_end = self.query_alignment_length = None
            if self.cigartuples:
                _, self.reference_length, self.query_alignment_length = sums(self.cigarstring)
                self.reference_end = self.reference_start + self.reference_length

        def infer_read_length(self):
            return sums(self.cigarstring)[0]

    class AlignmentFile:
        def __init__(self, path, mode="r", template=None, add_sam_header=None):
            self.path, self.mode = path, mode
            if "w" in mode:
                written[path] = []
                files[path] = (template.refs, written[path])
            self.refs, self.records = files[path]
            self.header = {"SQ": [{"SN": n, "LN": l} for n, l in self.refs]}

        def fetch(self, until_eof=False):
            return iter([r if isinstance(r, Aln) else Aln(r) for r in self.records])

        def write(self, aln):
            written[self.path].append(aln)

        def close(self):
            pass
    pysam = types.ModuleType("pysam")
    pysam.AlignmentFile = AlignmentFile
    sys.modules["pysam"] = pysam
    dumped = {}

    class KernelDensity:
        def __init__(self, bandwidth=1.0):
            self.bandwidth = bandwidth

        def fit(self, X):
            self.X = np.array(X)
            return self
    joblib = types.ModuleType("joblib")
    joblib.dump = lambda obj, path: dumped.__setitem__(os.path.basename(path), (obj.X, obj.bandwidth))
    sys.modules["joblib"] = joblib
    sk, skn = types.ModuleType("sklearn"), types.ModuleType("sklearn.neighbors")
    skn.KernelDensity = KernelDensity
    sk.neighbors = skn
    sys.modules["sklearn"], sys.modules["sklearn.neighbors"] = sk, skn
    return dumped, KernelDensity, joblib


def column(path):
    with open(path) as f:
        return [int(line.split("\t")[1]) for line in f]


def collect(dumped, work, prefix, two_d):
    """the lists of one head_align_tail run from what it handed to fit() and from its debugging files"""
    ints = lambda name: [int(v) for v in dumped[name][0][:, 0].tolist()]
    ht_log = dumped["training_ht_length.pkl"][0][:, 0]
    ht = np.rint(10.0 ** ht_log - 1).astype(np.int64)
    assert np.array_equal(np.log10(ht + 1), ht_log)                          # (what is stored are the integers)
    out = dict(aligned_ref_length=ints("training_aligned_region.pkl"), total_length=ints("training_aligned_reads.pkl"), ht_length=ht.tolist(),
               head_vs_ht_ratio=[float(v) for v in dumped["training_ht_ratio.pkl"][0][:, 0].tolist()])
    bws = [dumped["training_" + n + ".pkl"][1] for n in ("aligned_region", "aligned_reads", "ht_length", "ht_ratio")]
    assert bws == [10, 10, 0.01, 0.01], bws
    if os.path.exists(os.path.join(work, prefix + "_head.txt")) and os.path.getsize(os.path.join(work, prefix + "_head.txt")):
        out["head"], out["tail"] = column(os.path.join(work, prefix + "_head.txt")), column(os.path.join(work, prefix + "_tail.txt"))
        assert [h + t for h, t in zip(out["head"], out["tail"])] == out["ht_length"]
    if two_d:
        X, bw = dumped["training_aligned_region_2d.pkl"]
        out["rows_2d"], out["bw_2d"] = [[int(a), int(b)] for a, b in X.tolist()], float(bw)
        out["total_ref_length"] = [r[0] for r in out["rows_2d"]]
        assert [r[1] for r in out["rows_2d"]] == out["aligned_ref_length"]
    return out


def trx_input(seed=99):
    """(transcriptome records, genome records): reads in and not in the genome file, genome clips smaller and larger than the read's own"""
    rng = np.random.default_rng(seed)
    recs, genome = [], []
    tags = {"present": [], "absent": [], "genome_smaller": []}
    for i in range(48):
        name = "tread%03d" % i
        n = 2 if i % 6 == 1 else 1
        own = []
        for j in range(n):
            ref, total = TRX_REFS[int(rng.integers(0, 5))]
            ref_len = int(rng.integers(120, total - 100))
            h, t = int(rng.integers(0, 60)), int(rng.integers(0, 60))
            cigar = ("%dS" % h if h else "") + "%dM2D%dM" % (ref_len // 2, ref_len - ref_len // 2 - 2) + ("%dS" % t if t else "")
            flag = 16 if rng.random() < 0.4 else 0
            recs.append((name, flag, ref, int(rng.integers(1, total - ref_len)), cigar))
            own.append((t, h) if flag else (h, t))
        if i % 3 == 0:
            tags["absent"].append(name)
            continue
        tags["present"].append(name)
        for j in range(2 if i % 4 == 1 else 1):
            h = int(rng.integers(0, 25)) if i % 2 else int(rng.integers(40, 90))
            t = int(rng.integers(0, 90))
            flag = 16 if rng.random() < 0.4 else 0
            genome.append((name, flag, "chrA_1", int(rng.integers(1, 50000)), ("%dH" % h if h else "") + "300M500N200M" + ("%dS" % t if t else "")))
            gh = t if flag else h
            if gh < min(o[0] for o in own):
                tags["genome_smaller"].append(name)
    extra = [("gonly%02d" % i, 0, "chrB_1", 100 + i, "5S100M") for i in range(4)]
    genome = genome[:10] + extra + genome[10:]
    return recs, genome, tags


def maf_text(seed=3):
    """a <prefix>_besthit.maf: `s` lines in pairs as get_besthit_maf writes them (reference, then read)"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(40):
        aln, head = int(rng.integers(50, 3000)), int(rng.integers(0, 80)) * (i % 5 != 0)
        tail = int(rng.integers(0, 80)) * (i % 7 != 0)
        qaln = aln + int(rng.integers(-20, 20))
        out.append("s %s %d %d + %d %s\n" % (REFS[i % 3][0], int(rng.integers(0, 2000)), aln, REFS[i % 3][1], "ACGT-A"))
        out.append("s mread%02d %d %d %s %d %s\n" % (i, head, qaln, "+-"[i % 2], head + qaln + tail, "ACGTTA"))
    return "".join(out)


def main():
    sys.dont_write_bytecode = True
    files, written = {}, {}
    dumped, KernelDensity, joblib = install_standins(files, written)
    if REF_SRC not in sys.path:
        sys.path.insert(0, REF_SRC)
    import get_primary_sam as G
    import head_align_tail_dist as A
    assert A.KernelDensity is KernelDensity and A.joblib is joblib

    reads, tags = genome_input()
    primary = [r for read in reads for r in read]
    names = [r[0] for r in primary]
    index = {}
    for i, n in enumerate(names):
        index.setdefault(n, []).append(i)
    by_name = {n: [primary[i] for i in ix] for n, ix in index.items()}
    merges = lambda recs: [j for j in range(1, len(recs)) if recs[j][2] == recs[j - 1][2] and
                           ((edge_of(recs[0])[0] and edge_of(recs[j])[1]) or (edge_of(recs[0])[1] and edge_of(recs[j])[0]))]
    merges_prev = lambda recs: [j for j in range(1, len(recs)) if recs[j][2] == recs[j - 1][2] and
                                ((edge_of(recs[j - 1])[0] and edge_of(recs[j])[1]) or (edge_of(recs[j - 1])[1] and edge_of(recs[j])[0]))]
    # ---- the conditions on the input -----------------------------------------------------------------------------------------------
    assert 590 <= len(primary) <= 640 and 380 <= len(reads) <= 440, (len(primary), len(reads))
    assert len(tags["circ_SE"]) + len(tags["circ_ES"]) >= 20
    for n in tags["circ_SE"]:
        assert edge_of(by_name[n][0]) == (True, False) and edge_of(by_name[n][1]) == (False, True) and merges(by_name[n]) == [1]
    for n in tags["circ_ES"]:
        assert edge_of(by_name[n][0]) == (False, True) and edge_of(by_name[n][1]) == (True, False) and merges(by_name[n]) == [1]
    assert len(tags["triple"]) >= 5 and all(merges(by_name[n]) == [1, 2] for n in tags["triple"])
    no_merge = tags["wrong_edge"] + tags["len99"]
    assert len(no_merge) >= 5 and all(by_name[n][0][2] == by_name[n][1][2] and merges(by_name[n]) == [] for n in no_merge)
    assert any(sums(r[4])[1] == 99 for n in tags["len99"] for r in by_name[n])
    assert all(len(set(r[2] for r in by_name[n])) > 1 and 1 not in merges(by_name[n]) for n in tags["other_ref"])
    assert all(merges(by_name[n]) == [2] for n in tags["second_segment_grows"])
    assert len(tags["quirk"]) == 2 and all(merges(by_name[n]) != merges_prev(by_name[n]) for n in tags["quirk"])
    assert merges(by_name[tags["quirk"][0]]) == [] and merges_prev(by_name[tags["quirk"][0]]) == [2]
    assert merges(by_name[tags["quirk"][1]]) == [1] and merges_prev(by_name[tags["quirk"][1]]) == [1, 2]
    cig = [r[4] for r in primary]
    ends = lambda c: (OPS[cigartuples(c)[0][0]], OPS[cigartuples(c)[-1][0]])
    for a in "SH":
        assert any(ends(c)[0] == a and ends(c)[1] not in "SH" for c in cig) and any(ends(c)[1] == a and ends(c)[0] not in "SH" for c in cig)
        assert any(ends(c) == (a, a) for c in cig)
    assert any(c.startswith("5H10S") for c in cig)
    assert any(r[1] == 16 and ends(r[4])[0] in "SH" and ends(r[4])[1] in "SH" and cigartuples(r[4])[0][1] != cigartuples(r[4])[-1][1] for r in primary)
    assert all(any(op in c for c in cig) for op in "=XNP")
    assert any(len(cigartuples(c)) >= 5000 for c in cig) and any(n >= 100000000 for c in cig for _, n in cigartuples(c))
    assert index[names[0]] == [0] and index[names[-1]] == [len(primary) - 1]
    assert index[tags["across_block"][0]] == [255, 256, 257]
    assert names[-1] == tags["last_single"][0]

    everything = full_sam(reads)
    assert any(r[1] & 4 and r[5] == "*" for r in everything) and any(r[1] & 4 and r[5] != "*" for r in everything)
    assert any(r[1] & 256 for r in everything) and any(r[1] & 2048 for r in everything)
    files["training.sam"] = (REFS, everything)
    work = tempfile.mkdtemp(prefix="nsrl_")
    cwd = os.getcwd()
    try:
        os.chdir(work)
        # ---- genome mode: primary_and_unaligned, then head_align_tail on what it wrote ------------------------------------------------------
        unaligned_len, strandness, _ = G.primary_and_unaligned("training.sam", "training")
        kept = [a.rec[:5] for a in written["training_primary.bam"]]
        assert kept == primary
        num_aligned = A.head_align_tail("training", "bam", "genome")
        g = collect(dumped, work, "training", False)
        assert num_aligned == len(reads) == len(g["total_length"])
        pos = {n: i for i, n in enumerate(dict.fromkeys(names))}
        last, earlier, ht0 = pos[tags["last_single"][0]], pos[tags["head0_earlier"][0]], pos[tags["ht0"][0]]
        assert last == len(reads) - 1 and g["head"][last] == 0 and g["ht_length"][last] == 30 and g["head_vs_ht_ratio"][-1] == 0.0
        assert g["head"][earlier] == 0 and g["ht_length"][earlier] == 25 and g["ht_length"][ht0] == 0
        assert len(g["head_vs_ht_ratio"]) == sum(1 for h in g["head"][:-1] if h != 0) + 1
        assert g["head"][pos[tags["5H10S"][0]]] == 5 and g["tail"][pos[tags["5H10S"][0]]] == 8
        # ---- the two small texts: src/read_analysis.py:833-851 as it stands ------------------------------------------------------------------
        with open(os.path.join(REF_SRC, "read_analysis.py")) as f:
            lines = f.readlines()[832:851]
        assert "strandness_rate = open" in lines[0] and "alignment_rate.close()" in lines[-1]
        snippet = textwrap.dedent("".join(lines))
        texts = {}
        for key, ul in (("alignment_rate", unaligned_len), ("alignment_rate_all_aligned", np.array([], dtype=np.int64))):
            exec(snippet, dict(open=open, prefix="texts", strandness=strandness, unaligned_length=ul, num_aligned=num_aligned, numpy=np,
                               KernelDensity=KernelDensity, joblib=joblib, sys=sys, strftime=lambda fmt: ""))
            texts[key] = open("texts_reads_alignment_rate").read()
        texts["strandness"] = open("texts_strandness_rate").read()
        ul_X, ul_bw = dumped["texts_unaligned_length.pkl"]
        assert ul_bw == 10 and [int(v) for v in ul_X[:, 0].tolist()] == unaligned_len.tolist()
        # ---- transcriptome mode ------------------------------------------------------------------------------------------------------------------
        t_recs, t_genome, t_tags = trx_input()
        assert t_tags["present"] and t_tags["absent"] and t_tags["genome_smaller"]
        files["training_transcriptome_primary.bam"] = (TRX_REFS, [r + ("*",) for r in t_recs])
        files["training_genome_primary.bam"] = (REFS, [r + ("*",) for r in t_genome])
        dumped.clear()
        t_num = A.head_align_tail("training_transcriptome", "bam", "transcriptome")
        t = collect(dumped, work, "training", True)
        assert t_num == len(t["total_length"]) == 48 and len(t["rows_2d"]) == len(t_recs)
        # ---- MAF input ----------------------------------------------------------------------------------------------------------------------------
        maf = maf_text()
        files["maft_genome_primary.bam"] = (REFS, [])
        maf_out = {}
        for mode, prefix in (("genome", "mafg"), ("transcriptome", "maft_transcriptome")):
            with open(prefix + "_besthit.maf", "w") as f:
                f.write(maf)
            dumped.clear()
            n = A.head_align_tail(prefix, "maf", mode)
            dumped.update({k.replace("mafg_", "training_").replace("maft_", "training_"): v for k, v in list(dumped.items())})
            maf_out[mode] = collect(dumped, work, "none", mode == "transcriptome")
            assert n == 40
    finally:
        os.chdir(cwd)
        shutil.rmtree(work, ignore_errors=True)
    fixture = dict(refs=[list(r) for r in REFS], sam=sam_text(REFS, everything), primary=[list(r) for r in primary],
                   unaligned_len=[int(v) for v in unaligned_len.tolist()], strandness=float(strandness), genome=g, texts=texts,
                   tags={k: v for k, v in tags.items()},
                   trx=dict(refs=[list(r) for r in TRX_REFS], records=[list(r) for r in t_recs], genome_records=[list(r) for r in t_genome], **t),
                   maf=dict(text=maf, **maf_out))
    out = os.path.join(HERE, "reference_read_len.json.gz")
    with gzip.GzipFile(out, "wb", compresslevel=9, mtime=0) as f:
        f.write(json.dumps(fixture).encode())
    print("written", out, os.path.getsize(out), "bytes;", len(primary), "primary records in", len(reads), "reads;", len(everything), "records in all;",
          len(g["aligned_ref_length"]), "segments;", len(g["head_vs_ht_ratio"]), "ratios; strandness", strandness, texts)


if __name__ == "__main__":
    main()
