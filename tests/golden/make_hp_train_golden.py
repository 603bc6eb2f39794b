#!/usr/bin/env python3
"""Golden fixture of the training side's homopolymer-length model: the REAL reference's src/model_homopolymer_lengths.py —
analyze_homopolymers (H:36-139), calc_homopolymer_mis_rate (H:9-33) and fit_lr (H:189-201) — is run in the build container on a
synthetic MAF file for min_hp_len = 1, 3 and 5, and what it collects and writes is committed as data.

The module is imported unmodified; it imports `piecewise_regression`, which this image lacks and which none of the three functions
uses, so an empty stand-in module is registered under that name (fit_piecewise is NOT run: DESIGN §9 says what is written instead).
analyze_homopolymers reads field 7 of every line with split(), so an alignment without columns cannot be in its file: the fixture's
empty alignments are left out of the file the reference reads (they hold no homopolymer) and stay in the pairs.

Inputs: 65 random alignments each of 0, 1, 3, 10, 60 and 300 columns and three of about 5 000 — runs of 1 to 9 equal letters with about
10 % inserted, deleted and substituted bases (substitutions and a few reference letters are N or lower case) — and the hand-made corners
below, shuffled so that the lines begin at every offset mod 8 of the concatenated buffer.

    python tests/golden/make_hp_train_golden.py        -> tests/golden/reference_hp_train.json.gz
"""
import contextlib
import gzip
import io
import json
import os
import shutil
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF_SRC = "/root/reference/src"
KS = (1, 3, 5)


def segment_case(base, run, segment, left="C", right="T"):
    """a reference run of `run` letters whose span holds exactly `segment` as the read's bytes (dashes fill either line)"""
    n = max(run, len(segment))
    return (left + base * run + "-" * (n - run) + right, left + segment + "-" * (n - len(segment)) + right)


def corners():
    out = [
        ("AAAAAACGTCGTTTTTT", "AAAAAACGTCGTTTTTT"),          # a homopolymer as the first and as the last span of a line
        ("GGGGG-GACGTACCCCCCC", "GGGGGAGACGTAC-CCCCC"),
        ("------", "ACGTAA"),                                # dashes only
        ("", ""),                                            # no columns
        ("ACG--TTTTTT", "ACGTTTTTTTT"),                      # dashes in front that belong to the run (k > 1) / to G (k = 1)
        ("N---AAAAAAC", "NAATAAAAAAC"),
        ("AAAAAA--CCCCCC", "AAAAAAACCCCCCC"),                # dashes in front that belong to the previous homopolymer
        ("GTAA--CCCCCCC", "GTAACCCCCCCCC"),                  # a run too short, dashes, then a homopolymer
        ("GTAA--AAACCC--", "GTAAAAAA-CCCGG"),                # ... and one that goes on behind its dashes; dashes that end the line
        ("aaaaaaNNNNNNacgtTTTTTt", "aaaaaaNNNNNNacgtTTTTTt"),  # lower case and N never form one
        segment_case("A", 6, "AG"), segment_case("A", 6, "GA"), segment_case("A", 6, "AGA"), segment_case("A", 6, "AAGTAA"),
        segment_case("A", 6, "GAAAAG"), segment_case("A", 6, ""), segment_case("A", 6, "GGTC"), segment_case("G", 5, "aGGnGG"),
        segment_case("C", 5, "CCCCCCCCC"),                   # a read segment longer than the reference run
        segment_case("T", 7, "TTTATTTGTTTT", left="G", right="A"),
        ("C" + "A" * 150 + "-" * 20 + "A" * 150 + "T", "C" + "A" * 320 + "T"),      # beyond any LDS corner and beyond a first global cap
    ]
    assert all(len(r) == len(q) for r, q in out)
    return out


def random_pair(rng, n_cols):
    ref, qry = [], []
    letters = "ACGT"
    while len(ref) < n_cols:
        b = letters[int(rng.integers(0, 4))]
        for _ in range(int(rng.integers(1, 10))):
            u = rng.random()
            r = b if rng.random() >= 0.03 else ("N", b.lower())[int(rng.integers(0, 2))]
            if u < 0.10:
                ref.append("-"); qry.append(letters[int(rng.integers(0, 4))] if rng.random() < 0.5 else b)
            elif u < 0.20:
                ref.append(r); qry.append("-")
            elif u < 0.30:
                ref.append(r); qry.append("ACGTNacgt"[int(rng.integers(0, 9))])
            else:
                ref.append(r); qry.append(r)
    return "".join(ref[:n_cols]), "".join(qry[:n_cols])


def build_inputs(seed=20261018):
    """[(reference name, reference start, reference line, query line)]"""
    rng = np.random.default_rng(seed)
    pairs = corners()
    for n in (0, 1, 3, 10, 60, 300):
        pairs += [random_pair(rng, n) for _ in range(65)]
    pairs += [random_pair(rng, n) for n in (4997, 5003, 5010)]
    pairs = [pairs[i] for i in rng.permutation(len(pairs))]
    offsets = np.cumsum([0] + [len(r) for r, _ in pairs])[:-1]
    assert set(int(o) % 8 for o, (r, _) in zip(offsets, pairs) if r) == set(range(8))
    # few names and starts, so that equal rows of _hp_lengths.tsv occur (its Count column)
    return [("chr%d" % int(rng.integers(1, 4)), int(rng.integers(0, 3)) * 1000, r, q) for r, q in pairs]


def main():
    sys.dont_write_bytecode = True
    sys.modules["piecewise_regression"] = types.ModuleType("piecewise_regression")
    if REF_SRC not in sys.path:
        sys.path.insert(0, REF_SRC)
    import model_homopolymer_lengths as H

    records = build_inputs()
    work = tempfile.mkdtemp(prefix="nshp_")
    per_k = {}
    try:
        maf = os.path.join(work, "training.maf")
        with open(maf, "w") as f:
            for name, start, r, q in records:
                if r:
                    n, m = len(r.replace("-", "")), len(q.replace("-", ""))
                    f.write("s %s %d %d + 100000 %s\ns read 0 %d + %d %s\n" % (name, start, n, r, m, m, q))
        for k in KS:
            prefix = os.path.join(work, "k%d" % k)
            with contextlib.redirect_stdout(io.StringIO()):
                per_base, spans = H.analyze_homopolymers(maf, str(k), prefix)
                rate = H.calc_homopolymer_mis_rate(spans)
                header, lr = H.fit_lr(per_base)
            assert header == "intercept\tslope"
            per_k[str(k)] = dict(lengths={c: [[int(x), [int(v) for v in ys]] for x, ys in per_base[c].items()] for c in ("AT", "CG")},
                                 spans=[[a, b, c] for a, b, c in spans], mis_rate=rate, fit_lr=lr,
                                 lengths_file=open(prefix + "_hp_lengths.tsv").read())
            print("k = %d: %d homopolymers, mismatch rate %r, fit_lr %r" % (k, len(spans), rate, lr))
    finally:
        shutil.rmtree(work, ignore_errors=True)
    out = os.path.join(HERE, "reference_hp_train.json.gz")
    with gzip.open(out, "wt", compresslevel=9) as f:
        json.dump(dict(records=[list(r) for r in records], k=per_k), f)
    print("written", out, os.path.getsize(out), "bytes;", len(records), "alignments")


if __name__ == "__main__":
    main()
