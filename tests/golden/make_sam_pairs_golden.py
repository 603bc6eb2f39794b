#!/usr/bin/env python3
"""Golden fixture of the training side's SAM input ("SAM input: the line pairs"): SAM records whose aligned line pairs are
known, and the MAF text the REAL reference's src/pairwise2maf.py writes for them.

The records are the pairs of tests/golden/reference_hp_train.json.gz without the 66 that have no columns and the 7 whose query line is
only dashes (SAM can state neither): exactly 341 of 414 remain, and the script asserts that.  From each pair CIGAR, MD and SEQ are
derived — equal bytes are a match, case and `N` included; a mismatch puts the reference's byte into MD verbatim —, with soft clips of
0 / 3 / 17 bases in front and 0 / 1 / 40 behind on records whose first and last op is M (src/pairwise2maf.py:60, 67 takes the tail clip
as the text behind the last `M` and stops with ValueError otherwise), and FLAG 0 or 16 at random.

The expected text: the pairwise text `sam2pairwise` writes is restated here (four lines per record: the header fields, the read with its
clips, the match line, the reference with N over the clipped bases), and the unmodified pairwise2maf.main is run on it.  The script
asserts that every record comes back from it with exactly the two lines it was derived from.

    python tests/golden/make_sam_pairs_golden.py        -> tests/golden/reference_sam_pairs.json.gz
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
N_SOURCE, N_KEPT = 414, 341


def sam_fields(ref, qry):
    """(CIGAR, MD) of an aligned line pair"""
    ops, md, run = [], [], 0
    prev = None
    for r, q in zip(ref, qry):
        assert not (r == "-" and q == "-")
        op = "I" if r == "-" else "D" if q == "-" else "M"
        if ops and ops[-1][1] == op:
            ops[-1][0] += 1
        else:
            ops.append([1, op])
        if op == "M":
            if r == q:
                run += 1
            else:
                md.append(str(run) + r)
                run = 0
        elif op == "D":
            if prev == "D":
                md[-1] += r
            else:
                md.append(str(run) + "^" + r)
                run = 0
        if op != "I":                      # (an insertion does not appear in MD: a deletion run goes on behind it only in the CIGAR)
            prev = op
        else:
            prev = "I"
    md.append(str(run))
    return "".join("%d%s" % (n, op) for n, op in ops), "".join(md)


def main():
    sys.dont_write_bytecode = True
    with gzip.open(os.path.join(HERE, "reference_hp_train.json.gz"), "rt") as f:
        source = json.load(f)["records"]
    assert len(source) == N_SOURCE
    rng = np.random.default_rng(20261018)
    letters = "ACGT"
    records, lines, figures, index = [], [], [], []
    for i, (rname, start, ref, qry) in enumerate(source):
        if not ref or not qry.replace("-", ""):
            continue
        cigar, md = sam_fields(ref, qry)
        head = tail = 0
        if ref[0] != "-" and qry[0] != "-" and ref[-1] != "-" and qry[-1] != "-":
            head, tail = (0, 3, 17)[int(rng.integers(0, 3))], (0, 1, 40)[int(rng.integers(0, 3))]
        clip = lambda n: "".join(letters[int(x)] for x in rng.integers(0, 4, n))
        front, back = clip(head), clip(tail)
        seq = front + qry.replace("-", "") + back
        cigar = ("%dS" % head if head else "") + cigar + ("%dS" % tail if tail else "")
        records.append(["read%d" % i, (0, 16)[int(rng.integers(0, 2))], rname, start + 1, cigar, md, seq])
        lines.append([ref, qry])
        figures.append([head, tail, len(ref.replace("-", "")), len(qry.replace("-", ""))])
        index.append(i)
    assert len(records) == N_KEPT, len(records)
    offsets = np.cumsum([0] + [len(r) for r, _ in lines])[:-1]
    assert set(int(o) % 16 for o in offsets) == set(range(16))
    assert any(f[0] and f[1] for f in figures) and any(f[0] and not f[1] for f in figures) and any(f[1] and not f[0] for f in figures)

    if REF_SRC not in sys.path:
        sys.path.insert(0, REF_SRC)
    import pairwise2maf
    work = tempfile.mkdtemp(prefix="nssam_")
    try:
        pw, maf = os.path.join(work, "training_primary.out"), os.path.join(work, "training_processed.maf")
        with open(pw, "w") as f:
            for (qname, flag, rname, pos, cigar, md, seq), (ref, qry), (head, tail, _, _) in zip(records, lines, figures):
                n = len(seq)
                f.write("%s\t%d\t%s\t%d\t60\t%s\t*\t0\t0\n" % (qname, flag, rname, pos, cigar))
                f.write(seq[:head] + qry + seq[n - tail:] + "\n")
                f.write(" " * head + "".join("|" if a == b else " " for a, b in zip(ref, qry)) + " " * tail + "\n")
                f.write("N" * head + ref + "N" * tail + "\n")
        pairwise2maf.main(["-i", pw, "-o", maf])
        text = open(maf).read()
    finally:
        shutil.rmtree(work, ignore_errors=True)
    rows = text.split("\n")
    assert len(rows) == 2 * N_KEPT + 1 and rows[-1] == ""
    for k, (ref, qry) in enumerate(lines):
        assert rows[2 * k].split(" ")[6] == ref and rows[2 * k + 1].split(" ")[6] == qry, k
    out = os.path.join(HERE, "reference_sam_pairs.json.gz")
    with gzip.open(out, "wt", compresslevel=9) as f:
        json.dump(dict(records=records, lines=lines, figures=figures, source_index=index, maf=text), f)
    print("written", out, os.path.getsize(out), "bytes;", len(records), "records")


if __name__ == "__main__":
    main()
