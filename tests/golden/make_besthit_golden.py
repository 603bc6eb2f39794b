#!/usr/bin/env python3
"""Golden fixture of the training side's MAF input ("MAF input: the best hit per read"): the REAL reference's
src/get_besthit_maf.py (besthit_and_unaligned, G:8-56) is imported unmodified (it needs numpy and its own file_handler only) and run in
the build container on a synthetic LAST file; what it wrote and returned is committed as data.

The reference takes what `grep '^s '` leaves of LAST's output (src/read_analysis.py:187): the fixture stores the RAW file — with its
`#` headers, `a score=` lines and blank lines, and with `s` lines whose columns are separated by tabs — and this script hands the
reference the `s` lines of it (those that begin with `s` and a space or a tab: characterize.maf_pairs' filter), every line as it stands.
A '\\r' is not part of the fixture: the reference reads in text mode, which turns `\\r\\n` into `\\n` before anything is written, so
there is no file of the reference's to compare with (tests/test_besthit.py has that case hand-made).

The input: about 3 000 pairs over about 1 200 query names, and a reads file that also holds reads that never aligned.  Every case
named in main()'s asserts is present.

    python tests/golden/make_besthit_golden.py        -> tests/golden/reference_besthit.json.gz
"""
import gzip
import json
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF_SRC = "/root/reference/src"
REFS = [("chrA", 600000), ("chrB", 250000), ("chrC", 90000)]
LONG_NAME = "L" * 70


def seq_pair(rng, n):
    """two aligned lines of n columns: the query follows the reference with a few mismatches, insertions and deletions"""
    ref = rng.choice(list("ACGT"), n).tolist()
    qry = list(ref)
    for i in range(2, n - 2):
        u = rng.random()
        if u < 0.05:
            qry[i] = "ACGT"[("ACGT".index(ref[i]) + 1) % 4]
        elif u < 0.08 and ref[i - 1] != "-" and qry[i - 1] != "-":
            ref[i] = "-"
        elif u < 0.11 and ref[i - 1] != "-" and qry[i - 1] != "-":
            qry[i] = "-"
    return "".join(ref), "".join(qry)


class Maker:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.pairs = []                     # dicts, in file order

    def pair(self, qname, size, strands="++", style=0, cols=None, rname=None, **deco):
        r = self.rng
        rname, rtotal = (rname, 90000) if rname else REFS[int(r.integers(0, 3))]
        cols = int(r.integers(20, 60)) if cols is None else cols
        ref_seq, qry_seq = seq_pair(r, cols) if cols < 1000 else ("ACGTTGCA" * (cols // 8), "ACGTAGCA" * (cols // 8))
        head, tail = int(r.integers(0, 90)), int(r.integers(1, 90))
        return dict(qname=qname, size=size, strands=strands, style=style, rname=rname, rstart=int(r.integers(0, rtotal - 70000)),
                    rsize=sum(1 for c in ref_seq if c != "-"), rtotal=rtotal, head=head, total=head + size + tail, ref_seq=ref_seq, qry_seq=qry_seq, **deco)


def line(style, *fields):
    """one `s` line: style 0 single spaces, 1 LAST's padded columns, 2 tabs"""
    if style == 1:
        widths = (1, 14, 7, 5, 1, 7)
        return " ".join([str(f).ljust(w) if k == 1 else str(f).rjust(w) for k, (f, w) in enumerate(zip(fields[:6], widths))] + [fields[6]]) + "\n"
    return ("\t" if style == 2 else " ").join(str(f) for f in fields) + "\n"


def text_of(pairs):
    out = ["# LAST version 1256\n", "#\n", "# a=21 b=9 A=21 B=9 e=120\n", "# s this is a comment, not a line\n", "\n"]
    for k, p in enumerate(pairs):
        if p.get("a_line", k % 3 != 1):
            out.append("a score=%d EG2=0 E=0\n" % (p["size"] * 6))
        out.append(line(p["style"], "s", p["rname"], p["rstart"], p["rsize"], p["strands"][0], p["rtotal"], p["ref_seq"]))
        out.append(line(p["style"], "s", p["qname"], p["head"], p["size"], p["strands"][1], p["total"], p["qry_seq"]))
        if p.get("blank", k % 3 != 2):
            out.append("\n")
        if k % 500 == 17:
            out.append(" s indented: not a line\n")
            out.append("sx neither\n")
    text = "".join(out)
    assert text.endswith("\n")
    return text[:-1] if not pairs[-1].get("blank", (len(pairs) - 1) % 3 != 2) else text


def build_input():
    m = Maker(20261020)
    r = m.rng
    strands = lambda: ("++", "+-", "--")[int(r.integers(0, 3))]
    body = []
    for i in range(1180):                                          # the ordinary names: one to four pairs each, next to each other or not
        name = "rd%04d" % i
        for _ in range(int(r.choice([1, 1, 1, 2, 2, 3]))):
            body.append(m.pair(name, int(r.integers(30, 4000)), strands(), style=int(r.choice([0, 0, 1, 2]))))
    r.shuffle(body)
    hot = [m.pair("hot", int(r.integers(10, 900)), strands(), style=int(r.choice([0, 1]))) for _ in range(1000)]
    for k in (123, 456, 987):
        hot[k]["size"] = 950                                       # the maximum of the hot name, three times
    for h in hot:
        h["total"] = h["head"] + h["size"] + 5
    body[400:400] = hot[:600]                                      # 600 of them in one run, the rest spread over what follows
    rest = hot[600:]
    at = 1100
    for h in rest:
        body.insert(at, h)
        at += 3
    # ties of the maximum: first, more than 64 and more than 256 pairs further on; smaller sizes in front and in between
    for k, (pos, size) in enumerate(((50, 800), (60, 1234), (60 + 70, 1234), (60 + 70 + 300, 1234), (700, 1233))):
        body.insert(pos, m.pair("tie3", size, ("+-", "++", "--", "+-", "++")[k]))
    for pos in (5, 900, 1800, len(body) - 3):                      # one name scattered over the file
        body.insert(pos, m.pair("scattered", 500 + pos % 7, "+-"))
    # names that differ in the last byte only / of which one is the beginning of the other
    for k, name in enumerate(("read1", "read10", "read1x", "read1", "read1x", "read10")):
        body.insert(200 + 11 * k, m.pair(name, 100 + 10 * k, "++", style=k % 3))
    for k, name in enumerate((LONG_NAME + "a", LONG_NAME + "b", LONG_NAME + "a")):
        body.insert(300 + 40 * k, m.pair(name, 300 - k, "+-", style=1))
    body.insert(20, m.pair("nine_ten", 9, "++"))                   # 9 against 10: numbers, not text
    body.insert(25, m.pair("nine_ten", 10, "+-"))
    body.insert(30, m.pair("zero", 0, "--"))                       # size 0, alone and twice
    body.insert(31, m.pair("zero_twice", 0, "++"))
    body.insert(35, m.pair("zero_twice", 0, "+-"))
    body.insert(40, m.pair("single", 77, "++", style=2))
    body.insert(1000, m.pair("long_line", 59000, "+-", cols=59976, rname="chrOnlyRef"))          # two lines of 60 000 bytes
    body.append(m.pair("last_one", 321, "++", blank=False))        # the file ends without '\n'
    return body


def reads_text(pairs, seed=7):
    """the reads file: every query name (some over several lines, some with a description) and reads that never aligned"""
    rng = np.random.default_rng(seed)
    names = list(dict.fromkeys(p["qname"] for p in pairs))
    extra = ["never%03d" % i for i in range(60)] + ["chrOnlyRef", "chrA", "read", "read100", "rd", LONG_NAME, LONG_NAME + "c", "hot_", "ho"]
    everything = names + extra
    rng.shuffle(everything)
    out = []
    for k, n in enumerate(everything):
        head = ">" + n + ("" if k % 4 else " runid=%d  ch=%d" % (k, k % 512)) + ("\t" if k % 9 == 0 else "") + "\n"
        bases = "".join(rng.choice(list("ACGT"), int(rng.integers(1, 400))).tolist())
        out.append(head)
        if k % 3 == 0:                                              # several lines, a blank one among them every other time
            cut = sorted(set(int(x) for x in rng.integers(0, len(bases) + 1, 3)))
            parts = [bases[a:b] for a, b in zip([0] + cut, cut + [len(bases)])]
            if k % 2 == 0:
                parts.insert(1, "")
            out.extend(x + "\n" for x in parts)
        elif k % 3 == 1:
            out.append(bases + "  \n")                              # (trailing blanks: strip)
        else:
            out.append(bases + "\n")
    return "".join(out), set(extra)


def main():
    sys.dont_write_bytecode = True
    if REF_SRC not in sys.path:
        sys.path.insert(0, REF_SRC)
    import get_besthit_maf as G

    pairs = build_input()
    maf = text_of(pairs)
    reads, never = reads_text(pairs)
    # ---- the conditions on the input ---------------------------------------------------------------------------------------------------
    names = [p["qname"] for p in pairs]
    where = {}
    for i, n in enumerate(names):
        where.setdefault(n, []).append(i)
    sizes = lambda n: [pairs[i]["size"] for i in where[n]]
    assert 2900 <= len(pairs) <= 3300 and 1150 <= len(where) <= 1250, (len(pairs), len(where))
    assert where["single"] == [where["single"][0]] and len(where["hot"]) == 1000
    sc = where["scattered"]
    assert len(sc) == 4 and all(b - a > 256 for a, b in zip(sc, sc[1:]))
    assert all(len(where[n]) == 2 for n in ("read1", "read10", "read1x")) and all(len(where[LONG_NAME + c]) for c in "ab") and len(LONG_NAME) > 64
    t3 = where["tie3"]
    mx = max(sizes("tie3"))
    tied = [i for i in t3 if pairs[i]["size"] == mx]
    assert len(tied) == 3 and tied[0] != t3[0] and 64 < tied[1] - tied[0] < 256 < tied[2] - tied[1] and t3[-1] > tied[2]
    hmax = [i for i in where["hot"] if pairs[i]["size"] == 950]
    assert len(hmax) == 3 and max(sizes("hot")) == 950
    assert sizes("nine_ten") == [9, 10] and sizes("zero") == [0] and sizes("zero_twice") == [0, 0]
    assert set(p["strands"] for p in pairs) == {"++", "+-", "--"}
    assert set(p["style"] for p in pairs) == {0, 1, 2}
    lines = maf.split("\n")
    assert not maf.endswith("\n") and "\r" not in maf
    assert any(x.startswith("#") for x in lines) and any(x.startswith("a score=") for x in lines) and "" in lines[:-1]
    assert any(x.startswith(" s ") for x in lines) and any(x.startswith("sx ") for x in lines)
    assert any("   " in x for x in lines if x.startswith("s ")) and any(x.startswith("s\t") for x in lines)
    assert sum(1 for x in lines if len(x) + 1 >= 60000) == 2
    rd = reads.split("\n")
    assert any(x.startswith(">chrOnlyRef") for x in rd) and "chrOnlyRef" not in where and any(p["rname"] == "chrOnlyRef" for p in pairs)
    heads = [x.split()[0] for x in rd if x.startswith(">")]
    assert any(" runid=" in x for x in rd) and ">rd" in heads and ">" + LONG_NAME in heads
    s_only = "".join(x for x in maf.splitlines(True) if x.startswith("s ") or x.startswith("s\t"))
    assert s_only.count("\n") == 2 * len(pairs) - 1

    work = tempfile.mkdtemp(prefix="nsbh_")
    cwd = os.getcwd()
    try:
        os.chdir(work)
        with open("last_s_lines.maf", "w", newline="") as f:
            f.write(s_only)
        with open("reads.fasta", "w", newline="") as f:
            f.write(reads)
        unaligned_len, strandness = G.besthit_and_unaligned("reads.fasta", "last_s_lines.maf", "training")
        with open("training_besthit.maf", "rb") as f:
            besthit = f.read().decode()
    finally:
        os.chdir(cwd)
        shutil.rmtree(work, ignore_errors=True)
    # ---- what the reference did with the cases -----------------------------------------------------------------------------------------
    kept = besthit.splitlines(True)
    assert len(kept) == 2 * len(where) and not besthit.endswith("\n")
    kq = [x.split() for x in kept[1::2]]
    by = {q[1]: int(q[3]) for q in kq}
    first_max = sorted(next(j for j in where[n] if pairs[j]["size"] == max(sizes(n))) for n in where)       # (restated only for this assert)
    assert [q[1] for q in kq] == [names[i] for i in first_max]
    assert by["nine_ten"] == 10 and by["zero"] == 0 and by["tie3"] == mx and by["hot"] == 950 and by["last_one"] == 321
    tie_line = [x for x in kept[1::2] if x.split()[1] == "tie3"][0]
    assert tie_line.split()[4] == pairs[tied[0]]["strands"][1] and pairs[tied[0]]["strands"] != pairs[tied[1]]["strands"]
    n_seq_lines_unaligned = len(unaligned_len)
    assert 0 in unaligned_len.tolist() and n_seq_lines_unaligned > len(never)                       # blank lines and several lines per record
    fixture = dict(maf=maf, reads=reads, besthit=besthit, unaligned_len=[int(v) for v in unaligned_len.tolist()], strandness=float(strandness),
                   n_pairs=len(pairs), n_names=len(where), never=sorted(never))
    out = os.path.join(HERE, "reference_besthit.json.gz")
    with gzip.GzipFile(out, "wb", compresslevel=9, mtime=0) as f:
        f.write(json.dumps(fixture).encode())
    print("written", out, os.path.getsize(out), "bytes;", len(pairs), "pairs over", len(where), "names;", len(maf), "bytes of MAF;", len(kept) // 2,
          "kept; strandness", strandness, ";", len(unaligned_len), "unaligned sequence lines")


if __name__ == "__main__":
    main()
