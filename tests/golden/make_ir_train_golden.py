#!/usr/bin/env python3
"""Golden fixture of the training side's intron-retention model ("Intron retention: the Markov counts"): the REAL
reference's src/model_intron_retention.py (intron_retention, M:35-219) is run in the build container on a synthetic annotation and
synthetic alignments, and what it counts and writes is committed as data.

The module reads its annotation through HTSeq and its alignments through pysam, which this image lacks, so it is imported unmodified
with stand-ins: pysam.AlignmentFile serves fetch, is_unmapped, is_reverse, reference_name, query_name and get_blocks of SAM text;
HTSeq serves GFF_Reader(end_included=True), GenomicInterval and GenomicArrayOfSets("auto", stranded=False) with `+=` and
`[iv].steps()`.  What the steps of a real GenomicArrayOfSets look like depends on the order in which features were added; the
stand-in has two settings — the fewest steps (neighbours with equal sets are one step) and the most (a step ends at every boundary
of every feature) — and EVERY run below is made under both, with identical results asserted: the counts do not rest on where the steps
inside a stretch end.  dict_first_intron_state, dict_states and dict_ir_info are taken from the function's frame when it returns
(sys.setprofile): the files hold rounded ratios only.  Every read is also run alone, which gives the counts per read.

The input: about 300 reads over 13 annotated transcripts on three chromosomes (plus one chromosome without introns), with unmapped,
secondary, supplementary and repeated records.  Every branch named in the asserts of main() is present.

    python tests/golden/make_ir_train_golden.py        -> tests/golden/reference_ir_train.json.gz
"""
import gzip
import json
import os
import shutil
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF_SRC = "/root/reference/src"
STEPS = {"mode": "fewest"}


# ---- stand-ins -------------------------------------------------------------------------------------------------------------------------------
def install_standins():
    class GenomicInterval:
        def __init__(self, chrom, start, end, strand="."):
            self.chrom, self.start, self.end, self.strand = chrom, start, end, strand

        @property
        def length(self):
            return self.end - self.start

    class GenomicFeature:
        def __init__(self, name, type_, iv):
            self.name, self.type, self.iv, self.attr = name, type_, iv, {}

    class GFF_Reader:
        def __init__(self, path, end_included=False):
            assert end_included
            self.path = path

        def __iter__(self):
            with open(self.path) as f:
                for line in f:
                    if line == "\n" or line.startswith("#"):
                        continue
                    seqname, _, feature, start, end, _, strand, _, attr_str = line.split("\t", 8)
                    attr, first = {}, "_unnamed_"
                    for i, a in enumerate(attr_str.rstrip("\n").split(";")):       # (no quoted `;` in the synthetic annotation)
                        if not a.strip():
                            continue
                        key, _, val = a.strip().partition("=")
                        attr[key] = val
                        if i == 0:
                            first = val
                    ft = GenomicFeature(first, feature, GenomicInterval(seqname, int(start) - 1, int(end), strand))
                    ft.attr = attr
                    yield ft

    class View:
        def __init__(self, arr, iv):
            self.arr, self.iv = arr, iv

        def __iadd__(self, value):
            self.arr.feats.setdefault(self.iv.chrom, []).append((self.iv.start, self.iv.end, value))
            return self

        def steps(self):
            iv = self.iv
            feats = self.arr.feats.get(iv.chrom, [])                             # ("auto": an unknown chromosome is an empty one)
            cuts = sorted({iv.start, iv.end} | {p for s, e, _ in feats for p in (s, e) if iv.start < p < iv.end})
            segs = [[a, b, frozenset(v for s, e, v in feats if s <= a and b <= e)] for a, b in zip(cuts, cuts[1:])]
            if STEPS["mode"] == "fewest":
                merged = []
                for seg in segs:
                    if merged and merged[-1][2] == seg[2]:
                        merged[-1][1] = seg[1]
                    else:
                        merged.append(seg)
                segs = merged
            else:
                assert STEPS["mode"] == "most"
            STEPS["n"] = STEPS.get("n", 0) + len(segs)
            for a, b, fs in segs:
                yield GenomicInterval(iv.chrom, a, b, "."), set(fs)

    class GenomicArrayOfSets:
        def __init__(self, chroms, stranded=True):
            assert chroms == "auto" and stranded is False
            self.feats = {}

        def __getitem__(self, iv):
            return View(self, iv)

        def __setitem__(self, iv, view):
            assert isinstance(view, View)

    htseq = types.ModuleType("HTSeq")
    htseq.GenomicInterval, htseq.GFF_Reader, htseq.GenomicArrayOfSets = GenomicInterval, GFF_Reader, GenomicArrayOfSets
    sys.modules["HTSeq"] = htseq

    class Aln:
        def __init__(self, fld):
            self.query_name, self.flag, self.reference_name, self.pos, self.cigar = fld[0], int(fld[1]), fld[2], int(fld[3]), fld[5]
            self.is_unmapped, self.is_reverse = bool(self.flag & 4), bool(self.flag & 16)

        def get_blocks(self):
            out, pos, num = [], self.pos - 1, ""
            for c in self.cigar:
                if c.isdigit():
                    num += c
                    continue
                n, num = int(num), ""
                if c in "M=X":
                    out.append((pos, pos + n))
                    pos += n
                elif c in "DN":
                    pos += n
                else:
                    assert c in "ISHP"
            assert not num
            return out

    class AlignmentFile:
        def __init__(self, path, mode="r"):
            assert mode == "r"
            with open(path) as f:
                self.records = [Aln(l.rstrip("\n").split("\t")) for l in f if not l.startswith("@")]

        def fetch(self, until_eof=False):
            assert until_eof
            return iter(self.records)
    pysam = types.ModuleType("pysam")
    pysam.AlignmentFile = AlignmentFile
    sys.modules["pysam"] = pysam


# ---- the synthetic annotation --------------------------------------------------------------------------------------------------------------
# (id in the GFF, how the id is written, GFF chromosome, [(start, end) 0-based half-open, file order])
def annotation():
    t8 = [(20000 + 500 * i, 20000 + 500 * i + 50 + i) for i in range(40)]
    return [
        ("ENST00000001", "tid_version", "1", [(1000, 1200), (2000, 2300), (3000, 3100), (4000, 4180)]),
        ("ENST00000002", "parent_transcript", "chr2", [(5000, 5400), (5300, 5500), (7000, 7500)]),           # two that overlap; the union is as long as the third
        ("TX3", "parent_plain", "MT", [(100, 200), (200, 260), (400, 470)]),                                # two that touch
        ("TX4", "tid", "1", [(10000, 10500)]),
        ("TX5", "tid", "1", []),                                                                            # exon rows only
        ("ENST00000007", "tid_version", "chr2", [(12000, 12100), (12500, 12650), (13000, 13075)]),
        ("TX8", "tid", "chr2", t8),                                                                         # 40 introns: two words of a bit row
        ("TX9", "tid", None, [("1", 50000, 50100), ("chr2", 50000, 50150)]),                                # introns on two chromosomes
        ("TX10", "parent_plain", "MT", [(1000, 1100), (1500, 1620), (2000, 2140), (2600, 2760), (3300, 3480)]),
        ("TX11", "tid", "1", [(900, 1100), (1150, 2100), (2950, 3050)]),                                    # cuts the stretches of ENST00000001 into steps
        ("TX12", "tid", "chr2", [(30100, 30160), (30500, 30590), (30900, 30960)]),                          # first and last equally long; file order is not by start
        ("TX13", "tid", "chr2", [(90000, 90100), (91000, 91250)]),
        ("TXskipped", "id_first", "1", [(60000, 60100)]),                                                   # `ID=exon:..;Parent=..`: the rows do not resolve
    ]


def gff_text():
    rows = ["##gff-version 3\n", "\n"]
    for tid, how, chrom, introns in annotation():
        if how == "tid_version":
            attr = "ID=x;transcript_id=%s.5" % tid
        elif how == "tid":
            attr = "transcript_id=%s" % tid
        elif how == "parent_transcript":
            attr = "Parent=transcript:%s;Name=n" % tid
        elif how == "parent_plain":
            attr = "Parent=%s" % tid
        else:
            attr = "ID=exon:1;Parent=%s" % tid
        items = [(chrom, s, e) for s, e in introns] if chrom is not None else list(introns)
        if tid == "TX12":
            items = [items[1], items[0], items[2]]
        c0, s0 = (items[0][0], items[0][1]) if items else (chrom, 70000)
        rows.append("%s\tsyn\ttranscript\t%d\t%d\t.\t+\t.\t%s\n" % (c0, max(s0 - 299, 1), s0 + 30000, attr))
        rows.append("%s\tsyn\texon\t%d\t%d\t.\t+\t.\t%s\n" % (c0, max(s0 - 299, 1), max(s0, 1), attr))
        for c, s, e in items:
            rows.append("%s\tsyn\tintron\t%d\t%d\t.\t+\t.\t%s\n" % (c, s + 1, e, attr))
    rows.append("1\tsyn\tgene\t1\t99999\t.\t+\t.\tID=gene:G1\n")                                             # neither transcript_id nor Parent
    return "".join(rows)


SAM_CHROM = {"1": "chr1", "chr2": "chr2", "MT": "chrMTc"}      # GFF name -> RNAME: `chr1` against `1`; strip("chr") eats the c at the end of chrMTc


# ---- the reads -----------------------------------------------------------------------------------------------------------------------------------
def merge_ops(ops):
    out = []
    for n, c in ops:
        if out and out[-1][1] == c:
            out[-1][0] += n
        else:
            out.append([n, c])
    return "".join("%d%s" % (n, c) for n, c in out)


def random_read(rng, tid, chrom, introns):
    """an alignment along the transcript: per intron spliced out, read through, spliced a little short, or the end of the read"""
    union = []
    for s, e in sorted(introns):
        if union and s <= union[-1][1]:
            union[-1][1] = max(union[-1][1], e)
        else:
            union.append([s, e])
    k0 = int(rng.integers(0, len(union)))
    union = union[k0:k0 + int(rng.integers(1, 7))]
    start = max(union[0][0] - int(rng.integers(10, 150)), 1)
    pos, ops = start, []
    if rng.random() < 0.3:
        ops.append([int(rng.integers(1, 40)), "SH"[int(rng.integers(0, 2))]])

    def exon(to):
        nonlocal pos
        n = to - pos
        if n > 30 and rng.random() < 0.3:
            a = int(rng.integers(5, n - 10))
            if rng.random() < 0.5:
                ops.extend([[a, "M"], [int(rng.integers(1, 6)), "I"], [n - a, "M"]])
            else:
                d = int(rng.integers(1, min(6, n - a)))
                ops.extend([[a, "="], [d, "D"], [n - a - d, "M"]])
        elif n > 0:
            ops.append([n, "MX="[int(rng.integers(0, 3))] if rng.random() < 0.15 else "M"])
        pos = to
    ended = False
    for s, e in union:
        exon(s)
        u = rng.random()
        if u < 0.5:
            ops.append([e - s, "N"])
        elif u < 0.78:
            v = rng.random()
            if v < 0.2 and e - s > 20:
                a = int(rng.integers(5, e - s - 10))
                ops.extend([[a, "M"], [int(rng.integers(1, 5)), "I"], [e - s - a, "M"]])
            elif v < 0.4 and e - s > 20:
                a = int(rng.integers(5, e - s - 10))
                ops.extend([[a, "M"], [3, "D"], [e - s - a - 3, "M"]])
            else:
                ops.append([e - s, "M"])
        elif u < 0.9:
            cut = int(rng.integers(1, min(12, e - s)))
            ops.extend([[cut, "M"], [e - s - cut, "N"]] if rng.random() < 0.5 else [[e - s - cut, "N"], [cut, "M"]])
        else:
            ops.append([int(rng.integers(1, e - s + 1)), "M"])
            ended = True
            break
        pos = e
    if not ended:
        exon(pos + int(rng.integers(20, 150)))
    if rng.random() < 0.3:
        ops.append([int(rng.integers(1, 40)), "S"])
    return start, merge_ops(ops)


# hand-made reads: (tag, RNAME, 0-based start, CIGAR, transcript RNAME, retained introns, [first no, first IR, FF, FT, TF, TT])
def hand_reads():
    E1, E2, E3, E4 = (1000, 1200), (2000, 2300), (3000, 3100), (4000, 4180)
    T = "ENST00000001.2"
    return [
        ("run_ends_at_intron_end", "chr1", 900, "400M", T, [E1], [0, 1, 2, 0, 1, 0]),
        ("across_D", "chr1", 900, "150M20D230M", T, [E1], [0, 1, 2, 0, 1, 0]),                  # 50 + 130 = 180 = the fourth intron's length
        ("across_N", "chr1", 900, "150M20N230M", T, [E1], [0, 1, 2, 0, 1, 0]),
        ("across_I", "chr1", 900, "150M5I250M", T, [E1], [0, 1, 2, 0, 1, 0]),                   # 50 + 150 = 200
        ("pending_at_end", "chr1", 900, "300M", T, [], [1, 0, 3, 0, 0, 0]),
        ("partial_equals_none", "chr1", 1150, "300M", T, [], [1, 0, 3, 0, 0, 0]),
        ("partial_equals_other", "chr1", 1100, "300M", T, [E1], [0, 1, 2, 0, 1, 0]),            # 100 bases of the first = the third's length
        ("two_retained", "chr1", 900, "1500M", T, [E1, E2], [0, 1, 1, 0, 1, 1]),
        ("clips_and_pads", "chr1", 900, "7H12S100=3P300X9S", T, [E1], [0, 1, 2, 0, 1, 0]),
        ("boundary_of_next", "chrMTc", 50, "150M60N40M", "TX3", [(100, 200), (200, 260)], [0, 1, 0, 0, 1, 1]),     # 200 is the start of the second
        ("boundary_of_previous", "chrMTc", 200, "100M", "TX3", [(100, 200), (200, 260)], [0, 1, 0, 0, 1, 1]),     # 200 is the end of the first
        ("touching_pair", "chrMTc", 50, "250M", "TX3", [], [1, 0, 2, 0, 0, 0]),                            # one run of 160 over both
        ("overlapping_pair", "chr2", 4900, "700M", "ENST00000002", [(5000, 5400), (5300, 5500)], [0, 1, 0, 0, 1, 1]),
        ("pending_in_front_of_N", "chr2", 4900, "500M1000N", "ENST00000002", [], [1, 0, 2, 0, 0, 0]),
        ("other_chromosome", "chr2", 49900, "200M50N100M", "TX9", [(50000, 50100), (50000, 50150)], [0, 1, 0, 0, 0, 1]),
        ("no_intron_chromosome", "chr9", 900, "2500M", T, [], [1, 0, 3, 0, 0, 0]),
        ("transcript_without_introns", "chr1", 900, "400M", "TX5", [], [0, 0, 0, 0, 0, 0]),
        ("transcript_absent", "chr1", 900, "400M", "TX6", [], [0, 0, 0, 0, 0, 0]),
        ("transcript_rows_skipped", "chr1", 59900, "400M", "TXskipped", [], [0, 0, 0, 0, 0, 0]),
        ("single_intron", "chr1", 9900, "700M", "TX4", [(10000, 10500)], [0, 1, 0, 0, 0, 0]),
        ("word_border", "chr2", 35400, "1000M", "TX8", [(35500, 35581), (36000, 36082)], None),                # introns 31 and 32
        ("file_order", "chr2", 30000, "200M", "TX12", [(30100, 30160)], [1, 0, 0, 1, 1, 0]),                   # the second in file order
        ("equal_lengths", "chr2", 30800, "300M", "TX12", [(30900, 30960)], [1, 0, 1, 1, 0, 0]),                # as long as another: only positions decide
    ]


def build_input():
    rng = np.random.default_rng(20261019)
    ann = annotation()
    with_introns = [(tid, chrom, introns) for tid, how, chrom, introns in ann if introns and chrom is not None and how != "id_first"]
    g, t, tags = [], [], {}
    hand = hand_reads()
    n = 0

    def add(chrom, start, cigar, trx, flag=None, tag=None):
        nonlocal n
        n += 1
        q = "read%04d" % n
        flag = (16 if rng.random() < 0.4 else 0) if flag is None else flag
        g.append([q, flag, chrom, start + 1, cigar])
        t.append([q, 0, trx, int(rng.integers(1, 500)), "100M"])
        if tag:
            tags[tag] = q
        return q
    pending = list(hand)
    rng.shuffle(pending)
    while n < 290 or pending:
        if pending and (rng.random() < 0.12 or n >= 290):
            h = pending.pop()
            add(h[1], h[2], h[3], h[4], tag=h[0])
            continue
        tid, chrom, introns = with_introns[int(rng.integers(0, len(with_introns)))]
        start, cigar = random_read(rng, tid, chrom, introns)
        trx = tid + ".2" if tid.startswith("ENST") and rng.random() < 0.5 else tid
        add(SAM_CHROM[chrom], start, cigar, trx)
    # ---- the joins: what the two files hold beyond one record per read -------------------------------------------------------------------------
    g_by = {r[0]: i for i, r in enumerate(g)}
    # a read in only one of the two files
    tags["genome_only"] = add("chr1", 900, "400M", "ENST00000001")
    t.pop()
    tags["transcriptome_only"] = "tonly0001"
    t.append(["tonly0001", 0, "TX4", 5, "100M"])
    # a repeated QNAME in the genome file: the later record (no retention) replaces the earlier (retention); the place stays
    q = tags["dup_genome"] = tags["run_ends_at_intron_end"]
    g.append([q, 0, "chr1", 901, "300M"])
    # ... in the transcriptome file: the later record names another transcript
    q = tags["dup_transcriptome"] = tags["single_intron"]
    t.insert(3, [q, 0, "TX5", 9, "100M"])
    assert [r[0] for r in t].index(q) == 3 and sum(1 for r in t if r[0] == q) == 2 and [r for r in t if r[0] == q][-1][2] == "TX4"
    # secondary and supplementary records count like any other: a supplementary record behind the primary replaces it
    q = tags["supplementary_replaces"] = tags["two_retained"]
    g.append([q, 2048 | 16, "chr1", 1151, "300M"])
    q = tags["secondary_in_front"] = tags["across_I"]
    g.insert(g_by[q], [q, 256, "chr9", 5, "50M"])
    # unmapped records are skipped, wherever they stand
    g.append([tags["across_D"], 4, "*", 0, "*"])
    t.append([tags["across_D"], 4, "*", 0, "*"])
    g.insert(0, ["unmapped0", 4, "*", 0, "*"])
    tags["reverse"] = next(r[0] for r in g if r[1] == 16)
    return g, t, tags, hand


def sam_text(records, names):
    head = "@HD\tVN:1.6\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % (n, 10 ** 6) for n in names)
    return head + "".join("%s\t%d\t%s\t%d\t%d\t%s\t*\t0\t0\t*\t*\n" % (q, f, r, p, 0 if f & 4 else 60, c) for q, f, r, p, c in records)


G_NAMES = ("chr1", "chr2", "chrMTc", "chr9")
T_NAMES = ("ENST00000001.2", "ENST00000001", "ENST00000002.2", "ENST00000002", "ENST00000007.2", "ENST00000007", "TX3", "TX4", "TX5", "TX6", "TX8", "TX9",
           "TX10", "TX11", "TX12", "TX13", "TXskipped")


def run_reference(M, work, gff, g_records, t_records):
    """-> what intron_retention counts and writes for this input, identical under both step settings"""
    results = []
    for mode in ("fewest", "most"):
        STEPS["mode"] = mode
        with open(os.path.join(work, "g.sam"), "w") as f:
            f.write(sam_text(g_records, G_NAMES))
        with open(os.path.join(work, "t.sam"), "w") as f:
            f.write(sam_text(t_records, T_NAMES))
        taken = {}

        def prof(frame, event, arg):
            if event == "return" and frame.f_code.co_name == "intron_retention":
                loc = frame.f_locals
                taken["first"] = [loc["dict_first_intron_state"][False], loc["dict_first_intron_state"][True]]
                taken["states"] = [loc["dict_states"][k] for k in ((False, False), (False, True), (True, False), (True, True))]
                taken["ir_info"] = [[k, sorted(set(v))] for k, v in loc["dict_ir_info"].items() if v]
                taken["named"] = list(loc["dict_ir_info"])
        out = sys.stdout
        sys.stdout = open(os.devnull, "w")
        sys.setprofile(prof)
        try:
            M.intron_retention(os.path.join(work, "out"), gff, os.path.join(work, "g.sam"), os.path.join(work, "t.sam"))
        finally:
            sys.setprofile(None)
            sys.stdout.close()
            sys.stdout = out
        with open(os.path.join(work, "out_IR_markov_model")) as f:
            taken["markov_model"] = f.read()
        with open(os.path.join(work, "out_IR_info")) as f:
            taken["ir_info_text"] = f.read()
        results.append(taken)
    assert results[0] == results[1], "the result depends on where the steps end"
    return json.loads(json.dumps(results[0]))


def main():
    sys.dont_write_bytecode = True
    install_standins()
    if REF_SRC not in sys.path:
        sys.path.insert(0, REF_SRC)
    import model_intron_retention as M
    g, t, tags, hand = build_input()
    work = tempfile.mkdtemp(prefix="nsir_")
    try:
        gff = os.path.join(work, "annotation.gff3")
        with open(gff, "w") as f:
            f.write(gff_text())
        STEPS["n"] = 0
        full = run_reference(M, work, gff, g, t)
        n_fewest_and_most = STEPS["n"]
        # ---- every read alone: the final record of its QNAME in each file ------------------------------------------------------------------------
        last_g, last_t = {}, {}
        for r in g:
            if not r[1] & 4:
                last_g[r[0]] = r
        for r in t:
            if not r[1] & 4:
                last_t[r[0]] = r
        order = [q for q in last_g if q in last_t]
        per_read = []
        for q in order:
            one = run_reference(M, work, gff, [last_g[q]], [last_t[q]])
            retained = one["ir_info"][0][1] if one["ir_info"] else []
            per_read.append(dict(qname=q, counts=one["first"] + one["states"], retained=retained))
        assert [sum(p["counts"][i] for p in per_read) for i in range(6)] == full["first"] + full["states"]
        # ---- small cases: a sum of 0 in each of the three rows -------------------------------------------------------------------------------------
        small = {}
        for name, recs in (("start_row_0", [("chr1", 900, "400M", "TX5")]),
                           ("no_ir_row_0", [("chr2", 89900, "300M", "TX13")]),
                           ("ir_row_0", [("chr1", 900, "50M", "ENST00000001")]),
                           ("both_state_rows_0", [("chr1", 9900, "700M", "TX4"), ("chr1", 9900, "70M", "TX4")])):
            sg = [["s%d" % i, 0, c, s + 1, cg] for i, (c, s, cg, _) in enumerate(recs)]
            st = [["s%d" % i, 0, trx, 1, "100M"] for i, (_, _, _, trx) in enumerate(recs)]
            small[name] = dict(g_sam=sam_text(sg, G_NAMES), t_sam=sam_text(st, T_NAMES), **run_reference(M, work, gff, sg, st))
    finally:
        shutil.rmtree(work, ignore_errors=True)

    # ---- the conditions on the input ----------------------------------------------------------------------------------------------------------------
    by = {p["qname"]: p for p in per_read}
    pairs = lambda v: [list(x) for x in v]
    for tag, _, _, _, _, retained, counts in hand:
        q = tags[tag]
        if tag in ("run_ends_at_intron_end", "two_retained"):
            continue                                            # (replaced by a later record: below)
        if retained is not None:
            assert by[q]["retained"] == pairs(retained), (tag, by[q])
        if counts is not None:
            assert by[q]["counts"] == counts, (tag, by[q])
    # (boundary_of_next / boundary_of_previous: a run over ONE of two touching introns retains both — 200 lies on the inclusive end of
    # the first and on the start of the second)
    # one run of 160 over both touching introns: as long as neither, nothing retained
    assert by[tags["touching_pair"]] == dict(qname=tags["touching_pair"], counts=[1, 0, 2, 0, 0, 0], retained=[])
    assert by[tags["word_border"]]["counts"][1] == 0 and sum(by[tags["word_border"]]["counts"]) == 40
    # the joins
    assert tags["genome_only"] not in by and tags["transcriptome_only"] not in by
    assert by[tags["dup_genome"]]["counts"] == [1, 0, 3, 0, 0, 0] and order.index(tags["dup_genome"]) < len(order) - 3    # the later record; the first place
    assert by[tags["dup_transcriptome"]]["retained"] == [[10000, 10500]]
    assert by[tags["supplementary_replaces"]]["counts"] == [1, 0, 3, 0, 0, 0]
    assert by[tags["secondary_in_front"]]["retained"] == [[1000, 1200]]
    assert any(r[1] & 256 for r in g) and any(r[1] & 2048 for r in g) and any(r[1] == 16 for r in g) and any(r[1] & 4 for r in g)
    assert any(r[2].startswith("ENST") and r[2].endswith(".2") for r in t) and sum(by[tags["across_D"]]["counts"]) == 4
    assert 290 <= len(order) <= 330 and len(set(r[2] for r in g if not r[1] & 4)) == 4, len(order)
    assert sum(1 for p in per_read if len(p["retained"]) >= 2) >= 10 and sum(1 for p in per_read if p["retained"]) >= 60
    assert sum(1 for p in per_read if not p["retained"] and sum(p["counts"])) >= 60
    assert all(v > 0 for v in full["first"] + full["states"]), full
    assert full["named"][0] == last_t[order[0]][2].split(".")[0] and len(full["ir_info"]) >= 9
    assert small["start_row_0"]["markov_model"] == "succedent\tno_IR\tIR\nstart\t0.0\t0.0\nno_IR\t0.0\t0.0\nIR\t0.0\t0.0\n"
    assert small["no_ir_row_0"]["states"] == [0, 0, 1, 0] and small["ir_row_0"]["states"] == [3, 0, 0, 0]
    assert small["both_state_rows_0"]["first"] == [1, 1] and small["both_state_rows_0"]["states"] == [0, 0, 0, 0]
    assert n_fewest_and_most > 2 * len(order)

    fixture = dict(gff=gff_text(), g_sam=sam_text(g, G_NAMES), t_sam=sam_text(t, T_NAMES), order=order, per_read=per_read, tags=tags, small=small, **full)
    out = os.path.join(HERE, "reference_ir_train.json.gz")
    with gzip.GzipFile(out, "wb", compresslevel=9, mtime=0) as f:
        f.write(json.dumps(fixture).encode())
    print("written", out, os.path.getsize(out), "bytes;", len(order), "reads;", full["first"], full["states"], len(full["ir_info"]), "transcripts with retained introns")
    print(full["markov_model"])


if __name__ == "__main__":
    main()
