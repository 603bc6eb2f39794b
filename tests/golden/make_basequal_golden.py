#!/usr/bin/env python3
"""Golden fixture of the training side's base-quality model: the REAL reference's src/model_base_qualities.py —
analyze_aligned_base_qualities (M:55-79) and fit_lognorm (M:82-96) — is run in the build container on synthetic alignments, and what it
collects and writes is committed as data.

analyze_aligned_base_qualities reads `<prefix>_primary.bam` through pysam, which this image lacks; of an alignment it uses is_secondary,
query_name, get_tag('cs'), query_sequence, query_alignment_sequence / _start / _end and query_qualities / query_alignment_qualities, so
the module is imported unmodified with a pysam stand-in whose AlignmentFile serves those.  The cs strings are the ones of
make_hist_golden.py (oracle reads of the small test model + its hand-made cases) plus the corners of THIS walk; every alignment gets a
head and a tail clip of 0-40 bases (both zero on some), and every base a quality from a truncated log-normal of its class — a different
one per class, so that a class mix-up changes the fitted numbers — clipped to 1 .. 93, the values 1 and 93 present in every class.

    python tests/golden/make_basequal_golden.py        -> tests/golden/reference_basequal.json.gz
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
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
REF_SRC = "/root/reference/src"
TYPES = ("mis", "ins", "match", "ht", "unmapped")
# (mu, sd) of ln q per class: apart by more than any sampling error
DIST = {"mis": (2.2, 0.50), "ins": (2.4, 0.45), "match": (3.2, 0.35), "ht": (2.7, 0.60), "unmapped": (2.0, 0.40)}
N_READS = 50             # oracle reads behind the cs strings: every class stays below fit_lognorm's subsampling limit (asserted below)
N_UNMAPPED = 300


def draw(rng, name, n):
    mu, sd = DIST[name]
    return np.clip(np.rint(np.exp(rng.normal(mu, sd, n))), 1, 93).astype(np.int64)


def build_inputs(convert_cs, seed=777):
    """[(cs, qualities of the whole query, head, tail)] and the unmapped quality arrays"""
    from make_hist_golden import synthetic_cs
    rng = np.random.default_rng(seed)
    cases = [(cs, None) for cs in synthetic_cs(n_reads=N_READS)]
    # corners, (cs, aligned length or None = what the string covers): one op only; an error as first and as last aligned base; an
    # insertion run of more than 16 bases; junk between the items; a cs longer than the aligned part (cut inside a match and inside an
    # insertion); `-` and `=` items; an alignment that is all clip
    cases += [(":57", None), ("*ag", None), ("+acgt", None), ("*ag:5*ct", None), ("+a:5+c", None), ("+acg:20*ta", None),
              (":3+acgtacgtacgtacgtacgtacg:4", None), (":17+acgtacgtacgtacgtacgt:30", None), (":10+ACGT:5~gt12ag:6", None), ("x:4??*ag;:3", None),
              (":50*ag:50", 30), (":5+acgtacgt:5", 8), (":20*ag*ct:9", 21), (":6-acg:6-t*ag:2", None), (":4=ACG:2", None), (":12", 0), ("", 0)]
    alns = []
    for i, (cs, aligned) in enumerate(cases):
        arr = convert_cs(cs)
        if aligned is None:
            aligned = len(arr)
        kind = np.array([{":": "match", "+": "ins", "*": "mis"}[c] for c in arr[:aligned]], dtype=object)
        q = np.zeros(aligned, dtype=np.int64)
        for name in ("mis", "ins", "match"):
            sel = kind == name
            q[sel] = draw(rng, name, int(sel.sum()))
        if aligned == 0:
            head, tail = 7, 5                                             # all clip
        elif i % 5 == 0:
            head, tail = 0, 0
        else:
            head, tail = int(rng.integers(0, 41)), int(rng.integers(0, 41))
        alns.append((cs, np.concatenate([draw(rng, "ht", head), q, draw(rng, "ht", tail)]), head, tail))
    # the extreme values in every class: first / last aligned base of the first alignments that have the class there
    seen = set()
    for cs, q, head, tail in alns:
        arr = convert_cs(cs)
        n = len(q) - head - tail
        if n >= 2 and arr[0] == arr[n - 1] and arr[0] not in seen:
            seen.add(arr[0]); q[head] = 1; q[head + n - 1] = 93
        if head and tail and "ht" not in seen:
            seen.add("ht"); q[0] = 1; q[-1] = 93
    assert seen == {":", "+", "*", "ht"}, seen
    unmapped = [draw(rng, "unmapped", int(rng.integers(1, 400))) for _ in range(N_UNMAPPED)]
    unmapped[0][0] = 1; unmapped[0][-1] = 93
    return alns, unmapped


def main():
    sys.dont_write_bytecode = True

    class _Aln:
        def __init__(self, name, cs, q, head, tail, secondary=False):
            self.query_name, self._cs, self.is_secondary = name, cs, secondary
            self.query_qualities = q
            self.query_sequence = "A" * len(q)
            self.query_alignment_start, self.query_alignment_end = head, len(q) - tail
            self.query_alignment_sequence = self.query_sequence[head:len(q) - tail]
            self.query_alignment_qualities = q[head:len(q) - tail]

        def get_tag(self, tag):
            if tag != "cs":
                raise KeyError(tag)
            return self._cs

    served = []

    class _AlignmentFile:
        def __init__(self, path, mode):
            pass

        def __iter__(self):
            return iter(served)
    pysam = types.ModuleType("pysam")
    pysam.AlignmentFile = _AlignmentFile
    sys.modules["pysam"] = pysam
    if REF_SRC not in sys.path:
        sys.path.insert(0, REF_SRC)
    import model_base_qualities as MB

    alns, unmapped = build_inputs(MB.convert_cs)
    served += [_Aln("read%d" % i, cs, q, head, tail) for i, (cs, q, head, tail) in enumerate(alns)]
    served.insert(3, _Aln("secondary", ":5", np.full(5, 50, dtype=np.int64), 0, 0, secondary=True))      # skipped (M:66-68): not in the fixture
    quals = MB.analyze_aligned_base_qualities("training_primary.bam")
    quals["unmapped"] = [int(v) for u in unmapped for v in u.tolist()]                                    # src/get_primary_sam.py:172-175
    assert list(quals.keys()) == list(TYPES)
    for name in TYPES:
        assert 0 < len(quals[name]) <= 500000, (name, len(quals[name]))                                   # no np.random.choice in fit_lognorm
        assert min(quals[name]) == 1 and max(quals[name]) == 93, name                                     # no ln 0; the extremes are there
    work = tempfile.mkdtemp(prefix="nsbq_")
    try:
        MB.fit_lognorm(quals, os.path.join(work, "training"))
        text = open(os.path.join(work, "training_base_qualities_model_parameters.tsv")).read()
    finally:
        shutil.rmtree(work, ignore_errors=True)
    hist = {name: np.bincount(np.asarray(quals[name], dtype=np.int64), minlength=94).tolist() for name in TYPES}
    to_text = lambda q: "".join(chr(int(v) + 33) for v in q)
    out = os.path.join(HERE, "reference_basequal.json.gz")
    with gzip.open(out, "wt", compresslevel=9) as f:
        json.dump(dict(alignments=[[cs, to_text(q), head, tail] for cs, q, head, tail in alns], unmapped=[to_text(u) for u in unmapped],
                       hist=hist, file=text), f)
    print("written", out, os.path.getsize(out), "bytes;", len(alns), "alignments;", {k: len(v) for k, v in quals.items()})
    print(text)


if __name__ == "__main__":
    main()
