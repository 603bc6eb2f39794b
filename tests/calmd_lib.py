"""Test-side of the cs / MD stage (nanosim_amd/csrc/ns_calmd.h, nanosim_amd/characterize/calmd.py), sharing no code with either:
a generator of alignments over tests/golden/genome_small.fa that knows MD and cs by construction (from the events it draws, not from
the columns), an independent column-by-column writer of the rules, a plain restatement of the nine reasons a record is bad for with a
generator of corrupted records, and helpers that strip and re-tag SAM text."""
import os
import re

import numpy as np

from nanosim_amd import model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENOME = os.path.join(ROOT, "tests", "golden", "genome_small.fa")
KEPT = set("ACGTYRWSKMDVHBNX")            # what the engine's copy of a reference keeps after upper-casing; anything else is N there


def reference():
    return model.read_fasta(GENOME, "linear", raw_names=True)


def chromosomes(ref):
    """the chromosomes as the engine compares them: str each, upper case, N for what is no code"""
    out = []
    for i in range(len(ref.names)):
        t = ref.chrom(i).tobytes().decode("latin-1").upper()
        out.append("".join(c if c in KEPT else "N" for c in t))
    return out


# ---- the independent writer: one column after the other ------------------------------------------------------------------------------
def write_tags(cigar: str, pos: int, seq: str, chrom: str):
    """(MD, cs) of an alignment by the rules of ns_calmd.h; chrom: its chromosome as chromosomes() gives it"""
    r, q, u, m = pos - 1, 0, 0, 0
    md, cs = [], []

    def close():
        nonlocal m
        if m:
            cs.append(":%d" % m)
        m = 0
    for n, op in re.findall(r"(\d+)([MIDSH=X])", cigar):
        n = int(n)
        if op in "M=X":
            for _ in range(n):
                a, b = seq[q].upper(), chrom[r]
                if a == b and a != "N":
                    u += 1
                    m += 1
                else:
                    md.append("%d%s" % (u, b))
                    u = 0
                    close()
                    cs.append("*" + b.lower() + seq[q].lower())
                q += 1
                r += 1
        elif op == "I":
            close()
            cs.append("+" + seq[q:q + n].lower())
            q += n
        elif op == "D":
            md.append("%d^%s" % (u, chrom[r:r + n]))
            u = 0
            close()
            cs.append("-" + chrom[r:r + n].lower())
            r += n
        elif op == "S":
            q += n
    md.append("%d" % u)
    close()
    return "".join(md), "".join(cs)


# ---- the generator: truth from the events ---------------------------------------------------------------------------------------------
def _other(rng, b):
    return "ACGT".replace(b, "")[int(rng.integers(0, 3 if b in "ACGT" else 4))]


def alignment(rng, chroms, n_cols: int, kind: str, clips: bool = True, hard: bool = True, name: str = "r"):
    """one alignment of n_cols columns: dict(name, flag, chrom, pos, cigar, cigar_eqx, seq, md, cs).  kind: "clean" (no errors), "ont"
    (about 12 % errors), "alternate" (every other column a mismatch), "dense" and "wide" (an I or a D op between any two M ops, which are
    runs of 1-3 and of 60-70 columns).  The slice of the reference holds no N (a column on N is a
    mismatch whatever the read shows, which the hand-written cases cover)."""
    while True:
        ci = int(rng.integers(0, len(chroms)))
        chrom = chroms[ci]
        span = 4 * n_cols + 8 if kind == "dense" else n_cols + n_cols // 4 + 8         # (dense: up to three deleted letters per column)
        if span >= len(chrom):
            continue
        start = int(rng.integers(0, len(chrom) - span))
        if "N" not in chrom[start:start + span]:
            break
    events = []                         # ("=", L) | ("X", ref, read) | ("I", letters) | ("D", letters)
    r, cols = start, 0
    while cols < n_cols:
        if kind == "clean":
            step = ("=", n_cols - cols)
        elif kind == "alternate":
            step = ("X",) if cols % 2 else ("=", 1)
        elif kind in ("dense", "wide"):                  # an I or a D op between any two M ops: M runs of 1-3 columns, or of 60-70
            if events and events[-1][0] not in "ID":
                step = ("I",) if rng.random() < 0.5 else ("D",)
            else:
                run = int(rng.integers(1, 4)) if kind == "dense" else int(rng.integers(60, 71))
                k = min(run, n_cols - cols)
                step = ("X",) if k == 1 and rng.random() < 0.3 else ("=", k)
        else:
            x = rng.random()
            step = ("=", min(int(rng.geometric(0.12)), n_cols - cols)) if x < 0.5 else ("X",) if x < 0.7 else ("I",) if x < 0.85 else ("D",)
            if step[0] in "ID" and (not events or events[-1][0] in "ID"):
                step = ("=", 1)
        if step[0] == "=":
            events.append(("=", chrom[r:r + step[1]]))
            r += step[1]
            cols += step[1]
        elif step[0] == "X":
            events.append(("X", chrom[r], _other(rng, chrom[r])))
            r += 1
            cols += 1
        elif step[0] == "I":
            events.append(("I", "".join("ACGT"[int(k)] for k in rng.integers(0, 4, int(rng.integers(1, 4))))))
        else:
            n = int(rng.integers(1, 4))
            events.append(("D", chrom[r:r + n]))
            r += n
    if events[-1][0] in "ID":
        events.append(("=", chrom[r:r + 1]))
        r += 1
    head = "".join("ACGT"[int(k)] for k in rng.integers(0, 4, int(rng.integers(0, 9)))) if clips else ""
    tail = "".join("ACGT"[int(k)] for k in rng.integers(0, 4, int(rng.integers(0, 9)))) if clips else ""
    hard_head, hard_tail = (int(rng.integers(0, 3)), int(rng.integers(0, 3))) if clips and hard else (0, 0)
    seq, md, cs, ops, ops_eqx = [head], [], [], [], []
    u = m = 0

    def put(target, n, op):
        if target and target[-1][1] == op:
            target[-1][0] += n
        else:
            target.append([n, op])
    for e in events:
        if e[0] == "=":
            seq.append(e[1])
            u += len(e[1])
            m += len(e[1])
            put(ops, len(e[1]), "M")
            put(ops_eqx, len(e[1]), "=")
            continue
        if m:
            cs.append(":%d" % m)
        m = 0
        if e[0] == "X":
            seq.append(e[2])
            md.append("%d%s" % (u, e[1]))
            u = 0
            cs.append("*" + e[1].lower() + e[2].lower())
            put(ops, 1, "M")
            put(ops_eqx, 1, "X")
        elif e[0] == "I":
            seq.append(e[1])
            cs.append("+" + e[1].lower())
            put(ops, len(e[1]), "I")
            put(ops_eqx, len(e[1]), "I")
        else:
            md.append("%d^%s" % (u, e[1]))
            u = 0
            cs.append("-" + e[1].lower())
            put(ops, len(e[1]), "D")
            put(ops_eqx, len(e[1]), "D")
    md.append("%d" % u)
    if m:
        cs.append(":%d" % m)
    seq.append(tail)

    def text(o):
        body = "".join("%d%s" % (n, op) for n, op in o)
        return (("%dH" % hard_head if hard_head else "") + ("%dS" % len(head) if head else "") + body + ("%dS" % len(tail) if tail else "") +
                ("%dH" % hard_tail if hard_tail else ""))
    return dict(name=name, flag=16 if rng.random() < 0.5 else 0, chrom=ci, pos=start + 1, cigar=text(ops), cigar_eqx=text(ops_eqx), seq="".join(seq),
                md="".join(md), cs="".join(cs))


def random_records(seed: int = 20261020, n: int = 2000, max_cols: int = 3000, clips: bool = True, hard: bool = True):
    """n alignments of 1 .. max_cols columns in the three classes, a third each; lengths spread evenly over the decades"""
    rng = np.random.default_rng(seed)
    chroms = chromosomes(reference())
    out = []
    for i in range(n):
        cols = max(1, min(max_cols, int(round(10 ** rng.uniform(0, np.log10(max_cols))))))
        out.append(alignment(rng, chroms, cols, ("clean", "ont", "alternate")[i % 3], clips, hard, "read%d" % i))
    return out


# ---- SAM text ---------------------------------------------------------------------------------------------------------------------------
def sam_text(records, ref, tags: bool = True, eqx: bool = False, seed: int = 5, unmapped: int = 0) -> str:
    """SAM text of generated records under @SQ lines of the reference: with the generator's own MD:Z and cs:Z, or without; `unmapped`
    records (FLAG 4, with SEQ and QUAL) behind them"""
    rng = np.random.default_rng(seed)
    lengths = np.diff(ref.chrom_off.astype(np.int64)).tolist()
    out = ["@HD\tVN:1.6\tSO:unsorted\n"] + ["@SQ\tSN:%s\tLN:%d\n" % (n, l) for n, l in zip(ref.names, lengths)] + ["@PG\tID:aligner\tPN:aligner\n"]
    for r in records:
        qual = rng.integers(35, 75, len(r["seq"])).astype(np.uint8).tobytes().decode()
        line = "%s\t%d\t%s\t%d\t60\t%s\t*\t0\t0\t%s\t%s\tNM:i:0" % (r["name"], r["flag"], ref.names[r["chrom"]], r["pos"], r["cigar_eqx" if eqx else "cigar"],
                                                                   r["seq"], qual)
        if tags:
            line += "\tMD:Z:%s\tcs:Z:%s" % (r["md"], r["cs"])
        out.append(line + "\n")
    for i in range(unmapped):
        n = int(rng.integers(20, 60))
        out.append("unmapped%d\t4\t*\t0\t0\t*\t*\t0\t0\t%s\t%s\n" % (i, "".join("ACGT"[int(k)] for k in rng.integers(0, 4, n)),
                                                                    rng.integers(35, 75, n).astype(np.uint8).tobytes().decode()))
    return "".join(out)


def strip_tags(text: str) -> str:
    """the SAM text without any MD:Z or cs:Z field"""
    out = []
    for line in text.splitlines(True):
        if not line.startswith("@"):
            end = "\n" if line.endswith("\n") else ""
            f = line[:len(line) - len(end)].split("\t")
            line = "\t".join(f[:11] + [t for t in f[11:] if not t.startswith(("MD:Z:", "cs:Z:"))]) + end
        out.append(line)
    return "".join(out)


def retagged(text: str, ref) -> str:
    """the SAM text with MD:Z and cs:Z of the independent writer behind every mapped record that lacks them (MD first)"""
    chroms, index = chromosomes(ref), {n: i for i, n in enumerate(ref.names)}
    out = []
    for line in text.splitlines(True):
        f = line.rstrip("\n").split("\t")
        if not line.startswith("@") and len(f) >= 11 and not int(f[1]) & 4 and f[2] != "*" and f[5] != "*" and f[9] != "*":
            md, cs = write_tags(f[5], int(f[3]), f[9], chroms[index[f[2]]])
            end = "\n" if line.endswith("\n") else ""
            line = (line[:len(line) - len(end)] + ("" if any(t.startswith("MD:Z:") for t in f[11:]) else "\tMD:Z:" + md) +
                    ("" if any(t.startswith("cs:Z:") for t in f[11:]) else "\tcs:Z:" + cs) + end)
        out.append(line)
    return "".join(out)


# ---- bad records: the rules, one byte after the other ---------------------------------------------------------------------------------
MAX_DIGITS, MAX_OPLEN, MAX_TOTAL = 9, 1 << 28, 1 << 31


def bad_reason_at(cigar: str, seq, chrom: int, pos: int, chroms):
    """(reason, the CIGAR byte that decides or None) of a record by the rules of the opening comment of ns_calmd.h, 0: a good record.
    seq: bytes, or a str of code points below 256; chroms: as chromosomes() gives them.
    chrom, then POS; then the CIGAR byte by byte, the lowest byte that has a reason decides — at one op letter: it does not parse, the op
    is unknown, the order of the clips, the sums —, behind it digits at the end or no byte at all; then no column, the length of SEQ, the
    end of the chromosome, a SEQ byte."""
    sq = seq.encode("latin-1") if isinstance(seq, str) else bytes(seq)
    if chrom >= len(chroms):
        return 6, None
    if pos == 0:
        return 7, None
    digits = ""
    n_ops = 0
    columns = seq_sum = ref_sum = 0
    seen_aligned = lead_s = trail_s = closing_h = False                  # an M/I/D/=/X op; an S in front of them; one behind; an H that is not the first op
    for at, c in enumerate(cigar):
        if c.isascii() and c.isdigit():
            digits += c
            continue
        if not (c == "=" or (c.isascii() and c.isalpha())):
            return 1, at
        if not digits or len(digits) > MAX_DIGITS or int(digits) == 0 or int(digits) >= MAX_OPLEN:
            return 1, at
        if c not in "MIDSH=X":
            return 2, at
        n = int(digits)
        digits = ""
        # the clips: H only as the first or the last op, S only with nothing but an H between it and the end it stands at
        if closing_h:
            return 3, at                                                 # (an op behind an H that was not the first op)
        if c == "H":
            closing_h = n_ops > 0
        elif c == "S":
            if (trail_s if seen_aligned else lead_s):
                return 3, at
            if seen_aligned:
                trail_s = True
            else:
                lead_s = True
        else:
            if trail_s:
                return 3, at
            seen_aligned = True
        columns += n if c in "M=X" else 0
        seq_sum += n if c in "M=XIS" else 0
        ref_sum += n if c in "M=XD" else 0
        if max(columns, seq_sum, ref_sum) >= MAX_TOTAL:
            return 1, at
        n_ops += 1
    if digits or not cigar:
        return 1, len(cigar)
    if not columns:
        return 9, None
    if seq_sum != len(sq):
        return 4, None
    if pos - 1 + ref_sum > len(chroms[chrom]):
        return 8, None
    if not all(65 <= (b & 0xdf) <= 90 for b in sq):
        return 5, None
    return 0, None


def bad_reason(cigar: str, seq, chrom: int, pos: int, chroms) -> int:
    return bad_reason_at(cigar, seq, chrom, pos, chroms)[0]


CIGAR_NOISE, SEQ_NOISE = "0MIDSHNP=X,9m", "*=[`1"


def corrupted_records(seed: int = 20261021, n: int = 3000, max_cols: int = 400):
    """n records: good alignments of 1 .. max_cols columns with an indel between any two M runs ("dense" and "wide", in turn), each with
    one or two changes — a CIGAR byte replaced by one of CIGAR_NOISE, a SEQ byte by one of SEQ_NOISE, a digit appended to the CIGAR, a clip
    moved inward, POS pushed to the end of the chromosome; and, so that the set shows every reason, now and then the chromosome index set
    to the number of chromosomes or POS to 0.  [dict(cigar, seq: bytes, chrom, pos, reason, at, two)]: reason and at from bad_reason_at;
    two: the record has two changes in its CIGAR each of which alone is an error, of two different reasons at two different bytes."""
    rng = np.random.default_rng(seed)
    chroms = chromosomes(reference())
    out = []

    def cigar_byte(r):
        at = int(rng.integers(0, len(r["cigar"])))
        r["cigar"] = r["cigar"][:at] + CIGAR_NOISE[int(rng.integers(0, len(CIGAR_NOISE)))] + r["cigar"][at + 1:]

    def seq_byte(r):
        at = int(rng.integers(0, len(r["seq"])))
        r["seq"] = r["seq"][:at] + SEQ_NOISE[int(rng.integers(0, len(SEQ_NOISE)))] + r["seq"][at + 1:]

    def digit(r):
        r["cigar"] += "0123456789"[int(rng.integers(0, 10))]

    def clip(r):
        ops = re.findall(r"\d+[^\d]", r["cigar"])
        if len(ops) == len(re.findall(r"\d+[MIDSH=X]", r["cigar"])) and "".join(ops) == r["cigar"] and len(ops) >= 3:
            s = [i for i, o in enumerate(ops) if o[-1] in "SH"]
            i = s[int(rng.integers(0, len(s)))] if s else None
            if i is not None:
                o = ops.pop(i)
                ops.insert(int(rng.integers(1, len(ops))), o)
                r["cigar"] = "".join(ops)
                return
        cigar_byte(r)

    def end(r):
        span = sum(int(k) for k, o in re.findall(r"(\d+)([MD=X])", r["cigar"]))
        r["pos"] = max(1, len(chroms[min(r["chrom"], len(chroms) - 1)]) - span + 1 + int(rng.integers(0, 3)))

    def chrom(r):
        r["chrom"] = len(chroms)

    def pos0(r):
        r["pos"] = 0
    changes = [cigar_byte] * 10 + [seq_byte] * 3 + [digit] * 2 + [clip] * 2 + [end] * 2
    for i in range(n):
        cols = max(1, min(max_cols, int(round(10 ** rng.uniform(0, np.log10(max_cols))))))
        a = alignment(rng, chroms, cols, ("dense", "wide")[i % 2], name="c%d" % i)
        r = dict(cigar=a["cigar"], seq=a["seq"], chrom=a["chrom"], pos=a["pos"])
        first = chrom if i % 97 == 5 else pos0 if i % 97 == 6 else changes[int(rng.integers(0, len(changes)))]
        first(r)
        alone = [dict(r)]
        if rng.random() < 0.8:
            second = cigar_byte if first is cigar_byte and rng.random() < 0.8 else changes[int(rng.integers(0, len(changes)))]
            before = dict(r)
            second(r)
            if first is cigar_byte and second is cigar_byte and len(r["cigar"]) == len(a["cigar"]):
                # the second change alone, on the good record
                k = [j for j in range(len(r["cigar"])) if r["cigar"][j] != before["cigar"][j]]
                if len(k) == 1:
                    alone.append(dict(r, cigar=a["cigar"][:k[0]] + r["cigar"][k[0]] + a["cigar"][k[0] + 1:]))
        r["reason"], r["at"] = bad_reason_at(r["cigar"], r["seq"], r["chrom"], r["pos"], chroms)
        singles = [bad_reason_at(x["cigar"], x["seq"], x["chrom"], x["pos"], chroms) for x in alone]
        r["two"] = (len(singles) == 2 and all(s[0] in (1, 2, 3) and s[1] is not None for s in singles) and singles[0][0] != singles[1][0] and
                    singles[0][1] != singles[1][1])
        r["seq"] = r["seq"].encode("latin-1")
        out.append(r)
    return out
