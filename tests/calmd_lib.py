"""Test-side of the cs / MD stage (nanosim_amd/csrc/ns_calmd.h, nanosim_amd/characterize/calmd.py), sharing no code with either:
a generator of alignments over tests/golden/genome_small.fa that knows MD and cs by construction (from the events it draws, not from
the columns), an independent column-by-column writer of the rules, and helpers that strip and re-tag SAM text."""
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
    (about 12 % errors), "alternate" (every other column a mismatch).  The slice of the reference holds no N (a column on N is a
    mismatch whatever the read shows, which the hand-written cases cover)."""
    while True:
        ci = int(rng.integers(0, len(chroms)))
        chrom = chroms[ci]
        span = n_cols + n_cols // 4 + 8
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
