#!/usr/bin/env python3
"""Golden fixture of the training side's chimeric step ("Chimeric reads: the split-alignment choice"): the REAL reference's
src/get_primary_sam.py (primary_and_unaligned_chimeric, G:220-478) is run, unmodified, in the build container on synthetic alignments,
and what it collects is committed as data.

It reads its alignments through pysam, which this image lacks: the stand-in of make_read_len_golden.py is imported and its alignments get
what this function needs on top — get_tag (raising KeyError), query_alignment_start / query_alignment_end (the S ops among the leading
clips; start + M + I + `=` + X), query_alignment_qualities and query_length.  joblib.dump and KernelDensity are the recorders of that
script: the array handed to fit() is the fixture.  The function runs twice: with metagenome_list=None, and with a metagenome list so
that chimeric_species_count moves in both columns; EM_meta — the reference's quantification, not covered here — is stubbed with fixed
abundances.  log10 values are NOT stored: the script checks that the array handed to the gap KDE is np.log10(gap + 1) of the integers
it stores.

The input: about 300 reads on three references (two of one species; one of 5 000 bases), with unmapped reads, records of other reads and
unmatched records in between.  main() asserts, on a restatement of the choice that is used for nothing else and is itself checked against
what the reference wrote, that every branch named there occurs.

    python tests/golden/make_chimeric_train_golden.py        -> tests/golden/reference_chimeric_train.json.gz
"""
import gzip
import json
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_read_len_golden as RL                            # noqa: E402  (the pysam / joblib / sklearn stand-ins)

REF_SRC = RL.REF_SRC
REFS = [("spA_1", 60000), ("spA_2", 20000), ("spB_1", 5000)]
LN = dict(REFS)
ABUNDANCE = {"spA": 62.5, "spB": 37.5}


class Rec(tuple):
    """(qname, flag, rname, pos, cigar, seq) with .tags = {"NM": int, "SA": str}"""
    def __new__(cls, fields, tags):
        self = super().__new__(cls, fields)
        self.tags = tags
        return self


def parser_figures(cigar):
    """cigar_parser (G:16-31), restated only for the asserts on the input"""
    import re
    match = re.findall(r'(\d+)(\w)', cigar)
    qstart = int(match[0][0]) if match[0][1] in "SH" else 0
    qlen = sum(int(n) for n, o in match if o in "MI")
    rlen = sum(int(n) for n, o in match if o in "MD")
    return qstart, qstart + qlen, qlen, rlen


def pysam_figures(cigar):
    t = RL.cigartuples(cigar)
    qstart = 0
    for o, n in t:
        if RL.OPS[o] == "S":
            qstart += n
        elif RL.OPS[o] != "H":
            break
    _, rlen, qlen = RL.sums(cigar)
    return qstart, qstart + qlen, qlen, rlen


def edge_of(start, rlen, total):
    if rlen < 100:
        return (False, False)
    if start + rlen >= total - 1 - 400:
        return (False, True)
    return (start <= 400, False)


def overlap(a, b):
    return a[0] < b[1] - 10 and a[1] - 10 > b[0]


def trace(primary, species_of):
    """the choice for one primary Rec, restated for the asserts: a dict of what happened"""
    t = dict(has_sa="SA" in primary.tags, n_lists=1, alone=False, gaps=[], clamped=0, circular=[], joins=[], pieces=1, short_piece=False,
             ref_overlap_same=0, ref_overlap_other=0, tie=False, winner=0, no_primary=None, h_clip=False, eqx=False, keys=[], lost=False,
             same_species=0, other_species=0, same_qstart_sa=False, species_gaps=[])
    if not t["has_sa"]:
        return t
    q0, q1, qlen, rlen = pysam_figures(primary[4])
    ents = [dict(q=(q0, q1), r=(primary[3] - 1, primary[3] - 1 + rlen), score=qlen - primary.tags["NM"], rname=primary[2], d="-" if primary[1] & 16 else "+")]
    parts = primary.tags["SA"].split(";")
    t["lost"] = parts[-1] != ""
    for part in parts[:-1]:
        rname, pos, d, cigar, _, nm = part.split(",")
        s, e, ql, rl = parser_figures(cigar)
        ents.append(dict(q=(s, e), r=(int(pos) - 1, int(pos) - 1 + rl), score=ql - int(nm), rname=rname, d=d))
        t["h_clip"] |= cigar.split("H")[0].isdigit()
        t["eqx"] |= "=" in cigar or "X" in cigar
    lists = [[0]]
    for e in range(1, len(ents)):
        E = ents[e]
        took = 0
        for L in list(lists):
            q_ok = not any(overlap(E["q"], ents[m]["q"]) for m in L)
            r_same = any(overlap(E["r"], ents[m]["r"]) and ents[m]["rname"] == E["rname"] for m in L)
            r_other = any(overlap(E["r"], ents[m]["r"]) and ents[m]["rname"] != E["rname"] for m in L)
            if q_ok and r_same:
                t["ref_overlap_same"] += 1
            if q_ok and r_other and not r_same:
                t["ref_overlap_other"] += 1
            if q_ok and not r_same:
                L.append(e)
                took += 1
        t["joins"].append(took)
        if not took:
            lists.append([e])
    t["n_lists"] = len(lists)
    scores = [sum(ents[m]["score"] for m in L) for L in lists]
    w = scores.index(max(scores))
    t["winner"], t["tie"] = w, scores.count(max(scores)) > 1
    W = lists[w]
    if len(W) == 1 and ents[W[0]]["q"][0] != q0:
        t["alone"] = True
        return t
    order = sorted(W, key=lambda m: ents[m]["q"])
    t["pieces"] = len(order)
    t["same_qstart_sa"] = any(m != 0 and ents[m]["q"][0] == q0 for m in order)
    if not any(ents[m]["q"][0] == q0 for m in order):
        t["no_primary"] = ents[W[0]]["d"]
    pre = None
    for m in order:
        E = ents[m]
        edge = edge_of(E["r"][0], E["r"][1] - E["r"][0], LN[E["rname"]])
        if E["r"][1] - E["r"][0] < 100 and (E["r"][0] <= 400 or E["r"][1] >= LN[E["rname"]] - 401):
            t["short_piece"] = True
        if pre is not None:
            P, pedge = pre
            if E["rname"] == P["rname"] and ((pedge[0] and edge[1]) or (pedge[1] and edge[0])):
                t["circular"].append("SE" if pedge[0] else "ES")
            else:
                t["gaps"].append(max(0, E["q"][0] - P["q"][1]))
                t["clamped"] += E["q"][0] < P["q"][1]
                same = species_of(E["rname"]) == species_of(P["rname"])
                t["species_gaps"].append((species_of(P["rname"]), same))
                t["same_species" if same else "other_species"] += 1
        if E["q"][0] != q0:
            t["keys"].append((E["rname"], E["q"][0], E["q"][1], E["r"][0]))
        pre = (E, edge)
    return t


class Maker:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.n = 0

    def name(self):
        self.n += 1
        return "read%04d" % self.n

    def body(self, qlen, rlen=None, eqx=False):
        """ops with M + I = qlen and M + D = rlen (both as cigar_parser counts them); eqx: `=` and X ops in front, which it does not count"""
        r = self.rng
        ins = int(r.integers(1, 6)) if qlen > 60 else 0
        dele = (rlen - (qlen - ins)) if rlen is not None else int(r.integers(1, 6))
        if dele < 0:
            ins, dele = qlen - rlen, 0
        m = qlen - ins
        pre = "%d=%dX" % (int(r.integers(2, 30)), int(r.integers(1, 30))) if eqx else ""
        if m < 3:
            return pre + "%dM" % m + ("%dI" % ins if ins else "") + ("%dD" % dele if dele else "")
        a = int(r.integers(1, m - 1))
        b = int(r.integers(1, m - a))
        c = m - a - b
        return pre + "%dM" % a + ("%dI" % ins if ins else "") + "%dM" % b + ("%dD" % dele if dele else "") + ("%dM" % c if c else "")

    def mid(self, rname, rlen, slot):
        """a start away from both edges; different slots of one reference never overlap"""
        step = {"spA_1": 6000, "spA_2": 3000, "spB_1": 1300}[rname]
        return 600 + slot * step + int(self.rng.integers(0, 200))

    def piece(self, q0, qlen, rname, rstart, rev=None, nm=None, clip="S", rlen=None, eqx=False):
        rev = bool(self.rng.random() < 0.5) if rev is None else rev
        nm = int(self.rng.integers(0, 12)) if nm is None else nm
        return dict(q0=q0, qlen=qlen, rname=rname, rstart=rstart, rev=rev, nm=nm, clip=clip, rlen=rlen, eqx=eqx)

    def cigar(self, p, total):
        tail = total - p["q0"] - p["qlen"]
        assert tail >= 0
        return ("%d%s" % (p["q0"], p["clip"]) if p["q0"] else "") + self.body(p["qlen"], p["rlen"], p["eqx"]) + ("%d%s" % (tail, p["clip"]) if tail else "")

    def read(self, pieces, total=None, records=True, closing=True, secondary_copy=None, secondary_only=None):
        """[Rec]: the primary (pieces[0]) with its SA tag over pieces[1:] in that order, then a supplementary record per SA entry;
        secondary_copy: index of a piece that gets a second, secondary record with the same key behind its supplementary one;
        secondary_only: index of a piece whose only record is a secondary one"""
        name = self.name()
        total = total or max(p["q0"] + p["qlen"] for p in pieces) + int(self.rng.integers(0, 40))
        cig = [self.cigar(p, total) for p in pieces]
        tags = {"NM": pieces[0]["nm"]}
        if len(pieces) > 1:
            tags["SA"] = ";".join("%s,%d,%s,%s,60,%d" % (p["rname"], p["rstart"] + 1, "-" if p["rev"] else "+", c, p["nm"])
                                  for p, c in zip(pieces[1:], cig[1:])) + (";" if closing else "")
        out = [Rec((name, 16 if pieces[0]["rev"] else 0, pieces[0]["rname"], pieces[0]["rstart"] + 1, cig[0], "*"), tags)]
        if records:
            for i in range(1, len(pieces)):
                p = pieces[i]
                flag = (256 if secondary_only == i else 2048) | (16 if p["rev"] else 0)
                out.append(Rec((name, flag, p["rname"], p["rstart"] + 1, cig[i], "*"), {"NM": p["nm"]}))
                if secondary_copy == i:
                    out.append(Rec((name, 256 | (16 if p["rev"] else 0), p["rname"], p["rstart"] + 1, cig[i], "*"), {"NM": p["nm"] + 1}))
        return out


def scenarios(m):
    """{what: [reads]}; a read is a list of Rec"""
    r = m.rng
    S = {}

    def add(what, read):
        S.setdefault(what, []).append(read)
    for i in range(8):
        refs = [REFS[int(r.integers(0, 3))][0] for _ in range(3)]
        a = int(r.integers(300, 1500))
        # one compatible entry with a positive gap; the primary first or second along the read
        g = int(r.integers(11, 300))
        p, s = m.piece(0, a, refs[0], m.mid(refs[0], a, 0)), m.piece(a + g, 700, refs[1], m.mid(refs[1], 700, 2), clip="SH"[i % 2])
        add("positive_gap", m.read([p, s] if i % 2 else [dict(s, clip="S"), dict(p, clip="SH"[i % 4 == 0])]))
        # a query overlap of at most 10 bases: compatible, the negative gap is clamped to 0
        ov = int(r.integers(1, 11))
        add("clamped", m.read([m.piece(0, a, refs[0], m.mid(refs[0], a, 0)), m.piece(a - ov, 600, refs[1], m.mid(refs[1], 600, 2))]))
        # a query overlap above 10 opens a second list; the primary's list wins
        ov = int(r.integers(11, 200))
        add("second_list_loses", m.read([m.piece(0, a + 400, refs[0], m.mid(refs[0], a + 400, 0), nm=2), m.piece(a + 400 - ov, 250, refs[1], m.mid(refs[1], 250, 2), nm=9)]))
        # ... the second list wins alone: the primary record is kept alone
        big = "spA_1" if refs[1] == "spB_1" else refs[1]
        add("alone", m.read([m.piece(0, 300, refs[0], m.mid(refs[0], 300, 0), nm=5, rev=bool(i % 2)), m.piece(150, 900 + a, big, m.mid(big, 900 + a, 2), nm=3)]))
        # a score tie between the two lists: the first wins
        add("tie", m.read([m.piece(0, 500, refs[0], m.mid(refs[0], 500, 0), nm=4), m.piece(100, 506, refs[1], m.mid(refs[1], 506, 2), nm=10)]))
    for i in range(6):
        a = int(r.integers(400, 1200))
        # query-compatible, but the reference intervals overlap on the same reference: a second list
        st = m.mid("spA_1", a, 3)
        add("ref_overlap_same", m.read([m.piece(0, a, "spA_1", st, nm=1), m.piece(a + 50, 300, "spA_1", st + a // 2, rlen=300, nm=8)]))
        # ... on different references: compatible
        add("ref_overlap_other", m.read([m.piece(0, a, "spA_1", st), m.piece(a + 50, 300, "spA_2", st + a // 2, rlen=300)]))
        # an entry that joins two lists: B is compatible with the primary and with A, which overlaps the primary
        P, A = m.piece(0, 1000, "spA_1", m.mid("spA_1", 1000, 0), nm=3), m.piece(500, 700, "spA_2", m.mid("spA_2", 700, 1), nm=6)
        B = m.piece(1300 + int(r.integers(0, 90)), 800, "spB_1", m.mid("spB_1", 800, 2), nm=4)
        add("joins_two", m.read([P, A, B]))
        # a winning list of several pieces without the primary: the direction of its first-added entry counts
        P = m.piece(0, 400, "spA_2", m.mid("spA_2", 400, 0), nm=7, rev=bool(i % 2))
        A = m.piece(200, 1300, "spA_1", m.mid("spA_1", 1300, 1), nm=2, rev=i % 3 == 0)
        B = m.piece(1550, 900, "spB_1" if i % 2 else "spA_1", m.mid("spB_1", 900, 2) if i % 2 else m.mid("spA_1", 900, 4), nm=2, rev=i % 3 != 0)
        add("no_primary_%s" % ("-" if A["rev"] else "+"), m.read([P, A, B]))
    for i in range(6):
        ref = REFS[i % 3][0]
        total = LN[ref]
        a, b = int(r.integers(300, 900)), int(r.integers(300, 900))
        end = m.piece(0, a, ref, total - a - int(r.integers(0, 300)), rlen=a)
        start = m.piece(a + 20, b, ref, int(r.integers(0, 400)), rlen=b)
        # the two ends of a circular reference, in both orientations along the read: no gap is recorded
        add("circular_ES", m.read([end, start] if i % 2 else [start, end]))
        add("circular_SE", m.read([dict(start, q0=0), dict(end, q0=b + 20)] if i % 2 else [dict(end, q0=b + 20), dict(start, q0=0)]))
        # a piece under 100 reference bases is no edge: the gap is recorded
        add("short_piece", m.read([end, m.piece(a + 20, 99, ref, int(r.integers(0, 300)), rlen=99)]))
        add("short_piece", m.read([m.piece(0, 99, ref, total - 99 - int(r.integers(0, 200)), rlen=99), dict(start, q0=130)]))
        # three pieces: a circular join and a gap
        add("circular_then_gap", m.read([end, start, m.piece(a + b + 60, 500, "spA_1", m.mid("spA_1", 500, 5))]))
    for i in range(4):
        a = int(r.integers(300, 900))
        P, A = m.piece(0, a, "spA_1", m.mid("spA_1", a, 0)), m.piece(a + 30, 600, "spA_2", m.mid("spA_2", 600, 1), clip="H")
        add("h_clip", m.read([P, A]))
        add("eqx", m.read([P, dict(A, clip="S", eqx=True, rname="spB_1", rstart=m.mid("spB_1", 600, 1))]))
        add("secondary_matches", m.read([P, A], secondary_only=1))
        add("two_records_match", m.read([P, dict(A, clip="S")], secondary_copy=1))
        # an SA entry whose qstart is the primary's: the reference takes it for the primary record
        add("same_qstart", m.read([m.piece(0, 300, "spA_1", m.mid("spA_1", 300, 0), nm=9, rev=bool(i % 2)), m.piece(0, 1200, "spA_2", m.mid("spA_2", 1200, 1), nm=1)]))
        # a tag without the closing `;`: its last entry is lost
        add("lost_entry", m.read([P, A, m.piece(a + 700, 400, "spB_1", m.mid("spB_1", 400, 1))], closing=False))
        # four pieces, SA order unlike query order
        q = [0, 520, 1100, 1800]
        ps = [m.piece(q[j], 500, REFS[j % 3][0], m.mid(REFS[j % 3][0], 500, j)) for j in range(4)]
        add("four_pieces", m.read([ps[2], ps[3], ps[0], ps[1]]))
    return S


def build_input():
    m = Maker(20261019)
    S = scenarios(m)
    tags = {k: [read[0][0] for read in v] for k, v in S.items()}
    special = [read for v in S.values() for read in v]
    m.rng.shuffle(special)
    reads = []
    while special or len(reads) < 300:
        if special and (m.rng.random() < 0.45 or len(reads) >= 300):
            reads.append(special.pop())
        else:
            ref = REFS[int(m.rng.integers(0, 3))][0]
            a = int(m.rng.integers(200, 1500))
            read = m.read([m.piece(int(m.rng.integers(0, 60)), a, ref, m.mid(ref, a, int(m.rng.integers(0, 3))))])
            tags.setdefault("no_sa", []).append(read[0][0])
            reads.append(read)
    rng = np.random.default_rng(7)
    out = []
    k = 0
    for i, read in enumerate(reads):
        out.extend(read)
        u = rng.random()
        if u < 0.12:
            k += 1
            out.append(Rec(("unmapped%03d" % k, 4, "*", 0, "*", "*" if k % 7 == 3 else "ACGT" * int(rng.integers(1, 300)) + "A" * (k % 4)), {}))
        elif u < 0.2:                                       # a record of ANOTHER read's name, and one that matches nothing
            out.append(Rec(("stray%03d" % i, 2048, "spA_1", 777, "50S200M", "*"), {"NM": 3}))
        elif u < 0.26:
            out.append(Rec((read[0][0], 256 | (16 if u < 0.23 else 0), "spA_2", 888, "200M50H", "*"), {"NM": 0}))
    out.append(Rec(("unmapped_tail", 4, "*", 0, "*", "ACGTACGTAC"), {}))
    return reads, out, tags


def sam_text(refs, records):
    head = "@HD\tVN:1.6\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs) + "@PG\tID:synthetic\n"
    lines = []
    for rec in records:
        q, f, r, p, c, s = rec
        t = "".join("\t%s:%s:%s" % (k, "i" if k == "NM" else "Z", v) for k, v in rec.tags.items())
        lines.append("%s\t%d\t%s\t%d\t%d\t%s\t*\t0\t0\t%s\t*%s\n" % (q, f, r, p, 0 if f & 4 else 60, c, s, t))
    return head + "".join(lines)


def extend_standin():
    """what primary_and_unaligned_chimeric needs of an alignment on top of make_read_len_golden's stand-in"""
    import pysam
    base = pysam.AlignmentFile

    def more(a):
        tags = getattr(a.rec, "tags", {})

        def get_tag(name):
            if name not in tags:
                raise KeyError("tag '%s' not present" % name)
            return tags[name]
        a.get_tag = get_tag
        a.query_alignment_qualities = None
        if a.cigartuples:
            a.query_alignment_start, a.query_alignment_end = pysam_figures(a.cigarstring)[:2]
            assert a.query_alignment_end - a.query_alignment_start == a.query_alignment_length
        return a

    class AlignmentFile(base):
        def fetch(self, until_eof=False):
            return iter([more(a) for a in base.fetch(self, until_eof)])
    pysam.AlignmentFile = AlignmentFile


def run(G, dumped, written, metagenome_list):
    dumped.clear()
    unaligned_len, strandness, _ = G.primary_and_unaligned_chimeric("training.sam", "training", metagenome_list)
    X, bw = dumped["training_gap_length.pkl"]
    assert bw == 0.01 and X.shape[1] == 1
    gap = np.rint(10.0 ** X[:, 0] - 1).astype(np.int64)
    assert np.array_equal(np.log10(gap + 1), X[:, 0])                       # (what is stored are the integers)
    with open("training_chimeric_info") as f:
        info = f.read()
    return dict(gap_length=gap.tolist(), chimeric_info=info, strandness=float(strandness), unaligned_len=[int(v) for v in unaligned_len.tolist()],
                written=[list(a.rec) for a in written["training_primary.bam"]], written_nm=[a.rec.tags.get("NM") for a in written["training_primary.bam"]])


def main():
    sys.dont_write_bytecode = True
    files, written = {}, {}
    dumped, KernelDensity, joblib = RL.install_standins(files, written)
    extend_standin()
    if REF_SRC not in sys.path:
        sys.path.insert(0, REF_SRC)
    import get_primary_sam as G
    assert G.KernelDensity is KernelDensity and G.joblib is joblib
    seen = {}
    G.EM_meta = lambda quant_dic, all_species: dict(ABUNDANCE)

    reads, everything, tags = build_input()
    species_of = lambda name: "_".join(name.split("_")[:-1])
    T = {read[0][0]: trace(read[0], species_of) for read in reads}
    by = lambda what: [T[n] for n in tags[what]]
    # ---- the conditions on the input -----------------------------------------------------------------------------------------------------
    assert 290 <= len(reads) <= 330, len(reads)
    assert len(tags["no_sa"]) >= 100 and not any(t["has_sa"] for t in by("no_sa"))
    assert all(t["n_lists"] == 1 and t["pieces"] == 2 and t["gaps"] and t["gaps"][0] > 0 for t in by("positive_gap"))
    assert all(t["n_lists"] == 1 and t["gaps"] == [0] and t["clamped"] == 1 for t in by("clamped"))
    assert all(t["n_lists"] == 2 and t["winner"] == 0 and t["pieces"] == 1 and not t["alone"] and not t["gaps"] for t in by("second_list_loses"))
    assert all(t["n_lists"] == 2 and t["winner"] == 1 and t["alone"] for t in by("alone"))
    assert all(t["n_lists"] == 2 and t["tie"] and t["winner"] == 0 for t in by("tie"))
    assert all(t["ref_overlap_same"] == 1 and t["n_lists"] == 2 for t in by("ref_overlap_same"))
    assert all(t["ref_overlap_other"] == 1 and t["n_lists"] == 1 and t["pieces"] == 2 for t in by("ref_overlap_other"))
    assert all(t["joins"] == [0, 2] and t["n_lists"] == 2 for t in by("joins_two"))
    assert all(t["circular"] == ["ES"] and not t["gaps"] and t["pieces"] == 2 for t in by("circular_ES"))
    assert all(t["circular"] == ["SE"] and not t["gaps"] and t["pieces"] == 2 for t in by("circular_SE"))
    assert all(t["short_piece"] and not t["circular"] and len(t["gaps"]) == 1 for t in by("short_piece"))
    assert all(len(t["circular"]) == 1 and len(t["gaps"]) == 1 and t["pieces"] == 3 for t in by("circular_then_gap"))
    assert len(tags["no_primary_+"]) >= 2 and len(tags["no_primary_-"]) >= 2
    assert all(t["no_primary"] == "+" and t["winner"] == 1 and t["pieces"] == 2 for t in by("no_primary_+"))
    assert all(t["no_primary"] == "-" and t["winner"] == 1 and t["pieces"] == 2 for t in by("no_primary_-"))
    assert all(t["h_clip"] and t["pieces"] == 2 for t in by("h_clip")) and all(t["eqx"] and t["pieces"] == 2 for t in by("eqx"))
    assert all(t["same_qstart_sa"] and t["winner"] == 1 and t["pieces"] == 1 and not t["alone"] for t in by("same_qstart"))
    assert all(t["lost"] and t["pieces"] == 2 for t in by("lost_entry"))
    assert all(t["pieces"] == 4 and len(t["gaps"]) == 3 for t in by("four_pieces"))
    assert sum(t["same_species"] for t in T.values()) > 5 and sum(t["other_species"] for t in T.values()) > 5
    key_of = lambda rec: (rec[2],) + parser_figures(rec[4])[:2] + (rec[3] - 1,)
    for what, flags in (("secondary_matches", [256]), ("two_records_match", [2048, 256])):
        for read in [r for r in reads if r[0][0] in tags[what]]:
            k = T[read[0][0]]["keys"]
            assert len(k) == 1 and [rec[1] & ~16 for rec in read[1:] if key_of(rec) == k[0]] == flags
    assert any(r[1] & 4 and r[5] == "*" for r in everything) and any(r[1] & 4 and r[5] != "*" for r in everything)
    assert any(r[0].startswith("stray") for r in everything)

    files["training.sam"] = (REFS, everything)
    work = tempfile.mkdtemp(prefix="nsch_")
    cwd = os.getcwd()
    try:
        os.chdir(work)
        genome = run(G, dumped, written, None)
        median = G.median
        G.median = lambda v: seen.setdefault("betas", list(v)) and median(v)
        meta_list = {"spA": {}, "spB": {}}
        meta = run(G, dumped, written, meta_list)
        G.median = median
    finally:
        os.chdir(cwd)
        shutil.rmtree(work, ignore_errors=True)
    # ---- the restatement against what the reference did ------------------------------------------------------------------------------------
    names = [read[0][0] for read in reads]
    exp_gaps = [g for n in names for g in T[n]["gaps"]]
    assert genome["gap_length"] == exp_gaps == meta["gap_length"] and len(exp_gaps) > 60
    assert genome["written"] == meta["written"] and genome["strandness"] == meta["strandness"]
    n_written = {}
    for rec in genome["written"]:
        n_written[rec[0]] = n_written.get(rec[0], 0) + 1
    assert all(n_written[n] == T[n]["pieces"] for n in names) and [n for n in dict.fromkeys(r[0] for r in genome["written"])] == names
    for read in [r for r in reads if r[0][0] in tags["two_records_match"]]:          # the last matching record is the one written
        assert [rec[1] & ~16 for rec in genome["written"] if rec[0] == read[0][0]] == [0, 256]
    assert genome["chimeric_info"] == "Mean segments for each aligned read:\t" + str((len(exp_gaps) + len(reads)) / len(reads)) + "\n"
    # chimeric_species_count is a local of the function: it is taken from the restatement (keyed by the species of the PREVIOUS piece) and
    # checked through the list the reference hands to median()
    counts = {"spA": [0, 0], "spB": [0, 0]}
    for n in names:
        for sp, same in T[n]["species_gaps"]:
            counts[sp][0 if same else 1] += 1
    betas = [c[1] / (c[0] + c[1]) * 100 / (100 - ABUNDANCE[s]) for s, c in counts.items() if c[0] + c[1]]
    assert seen["betas"] == betas and all(c[0] and c[1] for c in counts.values())
    assert meta["chimeric_info"] == genome["chimeric_info"] + "Shrinkage rate (beta):\t" + str(median(betas))
    genome["species_count"] = {"spA": [0, 0], "spB": [len(exp_gaps), 0]}     # (genome mode: `species` stays the header loop's last, G:260)
    meta["species_count"] = {s: list(c) for s, c in counts.items()}
    fixture = dict(refs=[list(r) for r in REFS], sam=sam_text(REFS, everything), n_reads=len(reads), abundance=ABUNDANCE, genome=genome, meta=meta,
                   tags=tags, n_pieces=[T[n]["pieces"] for n in names])
    out = os.path.join(HERE, "reference_chimeric_train.json.gz")
    with gzip.GzipFile(out, "wb", compresslevel=9, mtime=0) as f:
        f.write(json.dumps(fixture).encode())
    print("written", out, os.path.getsize(out), "bytes;", len(reads), "reads;", len(everything), "records;", len(exp_gaps), "gaps;",
          len(genome["written"]), "written records; strandness", genome["strandness"], repr(meta["chimeric_info"]), meta["species_count"])


if __name__ == "__main__":
    main()
