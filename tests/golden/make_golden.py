#!/usr/bin/env python
"""Generate the golden fixtures under tests/golden/ by running the REAL reference.

Runs only in the build container (needs /root/reference); the fixtures it writes are plain data
(inputs + the reference's outputs) and are committed.  The reference is imported unmodified with the
three unused third-party modules stubbed; its random sources are wrapped to RECORD
the uniforms / run lengths it consumes so that oracle/ns_oracle.c can be replayed on the same tape.

    python tests/golden/make_golden.py [--dist-reads 100000]
"""
import argparse
import json
import multiprocessing as mp
import os
import random
import shutil
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from nanosim_amd import synth  # noqa: E402

REF_SRC = "/root/reference/src"
SMALL_SPEC = dict(n_train=2000, seed=7)
GENOME_SEED = 11
CHIMERIC_DENSE_MEAN = 2.0


class _GenomicIntervalRecord:
    """What the hot path uses of HTSeq.GenomicInterval: extract_read_pos constructs it from (chrom, start, end, strand) (S:178) and the
    worker reads those four attributes back (S:1162-1174).  A record with the same constructor lets the reference's own
    extract_read_pos run here (HTSeq itself is not in the image)."""
    def __init__(self, chrom, start, end, strand):
        self.chrom, self.start, self.end, self.strand = chrom, start, end, strand


def import_reference():
    for m in ("HTSeq", "pysam", "piecewise_regression"):
        sys.modules.setdefault(m, types.ModuleType(m))
    if not hasattr(sys.modules["HTSeq"], "GenomicInterval"):
        sys.modules["HTSeq"].GenomicInterval = _GenomicIntervalRecord
    sys.dont_write_bytecode = True
    if REF_SRC not in sys.path:
        sys.path.insert(0, REF_SRC)
    import simulator as S
    return S


def build_inputs(workdir):
    """Small model (text tables + npz committed; pickles only in workdir) and a 2-chromosome genome."""
    spec = synth.SynthModelSpec(**SMALL_SPEC)
    committed = os.path.join(HERE, "model_small", "training")
    synth.write_model(committed, spec, write_pkl=False, write_npz=True)
    prefix = os.path.join(workdir, "model", "training")
    synth.write_model(prefix, spec, write_pkl=True, write_npz=False)
    seq = synth.synth_sequence(180000, GENOME_SEED, n_frac=0.004, iupac_frac=0.002, lower_frac=0.08, hp_boost=0.02)
    recs = [("chr_A.1 first test chromosome", seq[:110000]), ("chrB", seq[110000:150000]), ("plasmid_c.2", seq[150000:])]
    fasta = os.path.join(HERE, "genome_small.fa")
    synth.write_fasta(fasta, recs)
    circ = os.path.join(HERE, "genome_circ.fa")
    synth.write_fasta(circ, [("NC_000913.3 synthetic circular", synth.synth_sequence(60000, GENOME_SEED + 1, iupac_frac=0.001))])
    return prefix, fasta, circ


class Recorder:
    """Wraps the reference's random sources and records what they return."""

    def __init__(self, S):
        self.S = S
        self.u, self.n = [], []
        self._rr = random.random
        self._pg, self._wg = S.mm.pois_geom, S.mm.wei_geom
        self._choice = random.choice
        self._uniform = random.uniform
        self._randint = random.randint

    def __enter__(self):
        S = self.S

        def rr():
            v = self._rr()
            self.u.append(v)
            return v

        def pg(*a):
            v = int(self._pg(*a))
            self.n.append(v)
            return v

        def wg(*a):
            v = int(self._wg(*a))
            self.n.append(v)
            return v

        def choice(seq):
            v = self._rr()
            self.u.append(v)
            return seq[int(v * len(seq))]

        def uniform(a, b):
            v = self._rr()
            self.u.append(v)
            return a + (b - a) * v

        def randint(a, b):
            v = self._rr()
            self.u.append(v)
            return a + int(v * (b - a + 1))

        random.random = rr
        random.choice = choice
        random.uniform = uniform
        random.randint = randint
        S.mm.pois_geom, S.mm.wei_geom = pg, wg
        return self

    def __exit__(self, *exc):
        random.random = self._rr
        random.choice = self._choice
        random.uniform = self._uniform
        random.randint = self._randint
        self.S.mm.pois_geom, self.S.mm.wei_geom = self._pg, self._wg


def edict_list(e_dict):
    return [[float(k), v[0], int(v[1])] for k, v in sorted(e_dict.items())]


def fixture_ecdf(S, prefix):
    out = {}
    for name in ("_first_match.hist", "_match_markov_model"):
        with open(prefix + name) as f:
            d = S.read_ecdf(f)
        out[name] = [{"bin": list(k1), "segs": [[k2[0], k2[1], v2[0], v2[1]] for k2, v2 in d[k1].items()]}
                     for k1 in d.keys()]
    return out


def fixture_error_list(S):
    cases = []
    seed = 100
    for m_ref in (1, 5, 60, 300, 3000, 8000):
        for fastq in (False, True):
            for rep in range(4):
                random.seed(seed); np.random.seed(seed); seed += 1
                with Recorder(S) as r:
                    l_new, middle_ref, e_dict, e_count = S.error_list(m_ref, S.match_markov_model, S.match_ht_list,
                                                                      S.error_par, S.trans_error_pr, fastq)
                cases.append(dict(m_ref=m_ref, fastq=fastq, u=r.u, n=r.n, l_new=int(l_new), middle_ref=int(middle_ref),
                                  e_dict=edict_list(e_dict),
                                  e_count=[int(e_count["match"]), int(e_count["mis"]), int(e_count["ins"])]))
    return cases


def fixture_mutate_read(S, genome):
    """error_list -> mutate_read on real reference sequence, letters driven by the recorded tape."""
    cases = []
    seed = 500
    for m_ref in (40, 300, 2500):
        for rep in range(4):
            random.seed(seed); np.random.seed(seed); seed += 1
            l_new, middle_ref, e_dict, e_count = S.error_list(m_ref, S.match_markov_model, S.match_ht_list,
                                                              S.error_par, S.trans_error_pr, False)
            start = 1000 + 37 * seed
            read = genome[start:start + middle_ref]
            log = _Log()
            with Recorder(S) as r:
                conv = S.case_convert(read)
                n_conv = len(r.u)
                out, quals = S.mutate_read(conv, "name", log, dict(e_dict), dict(e_count), False, None)
            cases.append(dict(read=read, converted=conv, e_dict=edict_list(e_dict), u_convert=r.u[:n_conv],
                              u_mutate=r.u[n_conv:], out=out, log=log.rows))
    # the survey's hand-made case
    read = "ACGTACGTAAAAAAGTCCGTAGCTAGGATC"
    e_dict = {3: ["mis", 2], 7.5: ["ins", 3], 8: ["del", 2], 15.5: ["ins", 1], 20: ["del", 1], 25: ["mis", 1]}
    for k in (None, 5):
        random.seed(9)
        log = _Log()
        with Recorder(S) as r:
            out, _ = S.mutate_read(read, "name", log, {a: list(b) for a, b in e_dict.items()},
                                   {"mis": 3, "ins": 4, "match": 22}, False, k)
        cases.append(dict(read=read, converted=read, e_dict=edict_list(e_dict), u_convert=[], u_mutate=r.u, out=out,
                          log=log.rows, k=k))
    return cases


class _Log:
    def __init__(self):
        self.rows = []

    def write(self, s):
        f = s.rstrip("\n").split("\t")
        self.rows.append([int(f[1]), f[2], int(f[3]), f[4], f[5]])


def fixture_mutate_fastq_classes(S, genome):
    """Quality CLASS of every emitted base: predict_base_qualities is replaced by a stub returning a
    per-class constant, so the positions of match/mis/ins qualities are captured exactly."""
    orig = S.model_base_quals.predict_base_qualities
    code = {}
    for cls, name in enumerate(("match", "mis", "ins", "ht", "unmapped")):
        code[S.lognorm_base_qual[name]["sd"]] = cls

    def stub(sd, loc, scale, n):
        return [code[sd]] * int(n)

    S.model_base_quals.predict_base_qualities = stub
    cases = []
    seed = 900
    try:
        for m_ref in (30, 400, 2000):
            for rep in range(3):
                random.seed(seed); np.random.seed(seed); seed += 1
                l_new, middle_ref, e_dict, e_count = S.error_list(m_ref, S.match_markov_model, S.match_ht_list,
                                                                  S.error_par, S.trans_error_pr, True)
                start = 2000 + 41 * seed
                conv = S.case_convert(genome[start:start + middle_ref])
                out, quals = S.mutate_read(conv, "name", None, dict(e_dict), dict(e_count), True, None)
                assert len(out) == len(quals)
                cases.append(dict(converted=conv, e_dict=edict_list(e_dict), classes=[int(q) for q in quals],
                                  out_len=len(out)))
    finally:
        S.model_base_quals.predict_base_qualities = orig
    return cases



def fixture_homopolymer(S, genome, k=5):
    """-k: mutate_read's homopolymer filter + mutate_homo, with every random source on tape.  Qualities are replaced by
    their CLASS (stub), np.random.normal is wrapped so that the sample each run consumed can be listed in run order."""
    import re as _re
    orig_q = S.model_base_quals.predict_base_qualities
    code = {S.lognorm_base_qual[name]["sd"]: cls for cls, name in enumerate(("match", "mis", "ins", "ht", "unmapped"))}
    S.model_base_quals.predict_base_qualities = lambda sd, loc, scale, n: [code[sd]] * int(n)
    orig_normal = np.random.normal
    cases = []
    seed = 2100
    pattern = "A{%d,}|C{%d,}|G{%d,}|T{%d,}" % (k, k, k, k)
    try:
        for m_ref in (60, 500, 3000, 6000):
            for rep in range(3):
                random.seed(seed); np.random.seed(seed); seed += 1
                l_new, middle_ref, e_dict, e_count = S.error_list(m_ref, S.match_markov_model, S.match_ht_list,
                                                                  S.error_par, S.trans_error_pr, True)
                start = 3000 + 53 * seed
                conv = S.case_convert(genome[start:start + middle_ref])
                log = _Log()
                with Recorder(S) as r1:
                    out1, q1 = S.mutate_read(conv, "name", log, {a: list(b) for a, b in e_dict.items()}, dict(e_count), True, k)
                calls = []

                def normal(mu, sigma, n):
                    v = orig_normal(mu, sigma, n)
                    calls.append((float(mu), float(sigma), [float(x) for x in v]))
                    return v

                np.random.normal = normal
                try:
                    with Recorder(S) as r2:
                        out2, q2 = S.mutate_homo(out1, list(q1), k)
                finally:
                    np.random.normal = orig_normal
                # which sample did each run use?  groups are created per length (first appearance) then A,T,C,G (S:639-650)
                runs = [(mt.start(), mt.end(), mt.group()[0]) for mt in _re.finditer(pattern, out1)]
                order, hist = [], {}
                for s0, e0, b in runs:
                    hist.setdefault(e0 - s0, {"A": 0, "T": 0, "C": 0, "G": 0})[b] += 1
                groups = {}
                ci = 0
                for length in hist:
                    for b in ("A", "T", "C", "G"):
                        if hist[length][b] > 0:
                            groups[(length, b)] = list(calls[ci][2]); ci += 1
                assert ci == len(calls)
                x_runs = []
                for s0, e0, b in runs:
                    x_runs.append(groups[(e0 - s0, b)].pop())          # consumed from the END (S:665-666)
                cases.append(dict(converted=conv, e_dict=edict_list(e_dict), k=k, u_mutate=r1.u, out1=out1,
                                  classes1=[int(x) for x in q1], log=log.rows, x_runs=x_runs, u_homo=r2.u, out2=out2,
                                  classes2=[int(x) for x in q2], runs=[[a, b_, c] for a, b_, c in runs]))
    finally:
        S.model_base_quals.predict_base_qualities = orig_q
    return cases

HP_EDGE_KS = (2, 3, 5, 8, 9, 16, 17)          # the switch points of the filter's window forms and of the run scan


def _hp_edge_runs(k, long_runs):
    """[(run length, injected draw or None)] of one hand-built mutate_homo input at k; None: the run is below k (no draw)"""
    if long_runs:
        runs = [(k, k + 1.0), (1100, 1100 + 16.0 if k in (5, 16) else 7.5), (k + 1, 0.5), (4200, 0.0), (64, 64 + 31.0), (k, k - 0.75), (130, 3.5)]
    else:
        ties = [n + 0.5 for n in range(6)]                                 # n even and odd: half to even decides
        runs = [(k, ties[0])]                                              # (the run at position 0)
        runs += [(k - 1, None), (k, ties[1]), (k + 1, ties[2])]
        runs += [(k, x) for x in ties[3:]]
        runs += [(k + 1, -0.0), (k, -1.75), (k + 2, 2.4999999999999996), (k + 2, 2.5000000000000004)]
        runs += [(k, k + 1.0), (k + 1, k + 1 + 15.0), (k, k + 16.0), (k + 1, k + 1 + 31.0), (k, k + 500.0)]
        for n in (15, 16, 17, 31, 32, 33, 63, 64, 65):
            runs.append((n, None if n < k else n + (-1.0, 0.25, 2.0)[n % 3]))
        runs += [(k, k - 0.25), (k + 3, k + 3 + 47.5), (65, 65 + 16.5), (33, 0.5), (k, float(k))]
    return [(n, x) for n, x in runs if n >= 1]


def _hp_edge_sequence(k, long_runs, rng):
    """the sequence and the draws of its runs (by run start): runs of _hp_edge_runs separated by 1 .. 3 bases without a repeat, plus
    adjacent runs of different bases, runs one base apart, N runs, a run at position 0 and a run at the last base"""
    seq, draws = [], {}

    def put_run(base, n, x):
        if n >= k and base != "N":
            draws[len(seq)] = x
        seq.extend(base * n)

    def put_gap(n, avoid):
        for i in range(n):
            seq.append(rng.choice([b for b in "ACGT" if b != seq[-1] and not (i == n - 1 and b == avoid)]))

    spec = _hp_edge_runs(k, long_runs)
    bases = "ATCG"
    for i, (n, x) in enumerate(spec):
        b = bases[i % 4]
        if i:
            put_gap(1 + i % 3 + (1 if seq[-1] == b else 0), b)
        put_run(b, n, x)
    if not long_runs:
        put_gap(2, "A")
        put_run("A", k, k - 1.0); put_run("C", k, k + 2.0); put_run("G", k + 1, 0.0); put_run("T", k, k + 17.0)      # AAAAACCCCC...: adjacent runs
        put_gap(2, "A")
        put_run("A", k, k + 1.0); put_run("C", 1, None); put_run("A", k, k - 1.0)                                      # one base apart
        put_run("G", 1, None); put_run("C", k + 1, 1.5)
        put_gap(1, "N")
        put_run("N", k, None); put_run("T", k, k + 1.5); put_run("N", k + 3, None); put_run("A", 1, None); put_run("N", 1, None)
        put_gap(2, "C")
    else:
        put_gap(3, "C")
    put_run("C", k + 1, k + 1 + 16.0)                                      # (the run at the last base)
    return "".join(seq), draws


def _hp_edge_filter_case(k, variant, rng):
    """a read and a hand-made e_dict around its runs: every type ending exactly where a run starts and starting exactly where it ends, on
    its first and last base, insertions whose float key (pos - 1/2, S:1929-1937) alone decides, events at position 0 and on the last base,
    and the read's ends cutting a run to k - 1 (variant 0) or leaving exactly k (variant 1)"""
    seq, e_dict = [], {}

    def gap(n, avoid):
        for i in range(n):
            seq.append(rng.choice([b for b in "ACGT" if not (seq and b == seq[-1]) and not (i == n - 1 and b == avoid)]))

    def ev(pos, ty, n):
        key = pos - 0.5 if ty == "ins" else pos
        assert key not in e_dict and 0 <= pos
        e_dict[key] = [ty, n]

    edge = k - 1 + variant
    seq.extend("A" * edge)                                                 # the run the read's start cuts (or not)
    ev(0, ("mis", "ins", "del")[k % 3], 1)
    gap(14, "C")
    placements = []
    for ty in ("mis", "ins", "del"):
        for where in ("before_kept", "before_hit", "first", "inside", "last", "after_hit", "after_kept"):
            placements.append((ty, where))
    for i, (ty, where) in enumerate(placements):
        b = "CGTA"[i % 4]
        n_run = k + (i % 2)
        s = len(seq); e = s + n_run
        seq.extend(b * n_run)
        n = 2 + (i % 2)
        if where == "before_kept":
            ev(s - n, ty, n)                                               # mis / del: [s - n, s); ins: ends 1/2 before the run
        elif where == "before_hit":
            ev(s - n + 1, ty, n)                                           # reaches base s; ins: only through a base beyond pos
        elif where == "first":
            ev(s, ty, 1)
        elif where == "inside":
            ev(s + n_run // 2, ty, 1)
        elif where == "last":
            ev(e - 1, ty, 1)
        elif where == "after_hit":
            ev(e if ty == "ins" else e - 1, ty, n)                         # ins at pos = e: only base pos - 1 is in the run
        else:
            ev(e + 1 if ty == "ins" else e, ty, n)
        gap(13 + i % 3, "CGTA"[(i + 1) % 4])
    gap(1, "T")
    last = len(seq) + edge - 1
    seq.extend("T" * edge)                                                 # the run the read's end cuts (or not)
    ev(last, "del" if k % 2 else "mis", 1)
    read = "".join(seq)
    n_mis = sum(v[1] for v in e_dict.values() if v[0] == "mis")
    n_ins = sum(v[1] for v in e_dict.values() if v[0] == "ins")
    n_del = sum(v[1] for v in e_dict.values() if v[0] == "del")
    return read, e_dict, {"mis": n_mis, "ins": n_ins, "match": len(read) - n_mis - n_del}


# the counters (tests/oracle_lib.py HP_COUNTERS) the fixture is there to raise when the oracle replays it
HP_EDGE_HOMO_COUNTERS = ("runs", "grow", "grow_15", "shrink", "shrink_4095", "size0", "l64", "l1024", "l4096", "at_start", "at_end",
                         "mis2", "mis_appended", "mis_mid_ins", "edits3", "tie", "adjacent")
HP_EDGE_FILTER_COUNTERS = ("drop_mis", "drop_ins", "drop_del", "keep_mis", "keep_ins", "keep_del", "ins_key_before", "ins_key_beyond",
                           "near_end", "run_cut")


def fixture_hp_edges(S):
    """-k at the branches the sampled tapes of fixture_homopolymer do not reach: hand-built inputs at the k where the engine's kernels
    switch form, mutate_homo with INJECTED np.random.normal draws (ties n + 1/2, -0.0, negative, growth by 1 .. 500, a 4200-base run
    re-sampled to 0) at two mismatch rates, and hand-made e_dicts for mutate_read's filter.  Only the inputs and what the reference
    returned are kept; get_nd_par is replaced (its values do not matter once the draws are injected)."""
    import re as _re
    orig_q = S.model_base_quals.predict_base_qualities
    code = {S.lognorm_base_qual[name]["sd"]: cls for cls, name in enumerate(("match", "mis", "ins", "ht", "unmapped"))}
    S.model_base_quals.predict_base_qualities = lambda sd, loc, scale, n: [code[sd]] * int(n)
    orig_normal, orig_par, orig_rate = np.random.normal, S.model_hp_len.get_nd_par, S.hp_mis_rate
    S.model_hp_len.get_nd_par = lambda length, pw, lr: (float(length), 1.0) * 4
    homo, filt = [], []
    rng = random.Random(4100)
    try:
        for k in HP_EDGE_KS:
            pattern = "A{%d,}|C{%d,}|G{%d,}|T{%d,}" % (k, k, k, k)
            for long_runs in (False, True):
                for rate in ((0.03, 0.5) if not long_runs else (0.5,) if k in (3, 8, 16) else (0.03,)):
                    seq, draws = _hp_edge_sequence(k, long_runs, rng)
                    assert len(seq) <= 6000, len(seq)
                    runs = [(mt.start(), mt.end(), mt.group()[0]) for mt in _re.finditer(pattern, seq)]
                    assert [r[0] for r in runs] == sorted(draws), "the hand-built runs are not the runs the reference finds"
                    # the groups np.random.normal is asked for (S:639-650): per length in order of first appearance, then A, T, C, G;
                    # every group is consumed from the END (S:665-666)
                    hist = {}
                    for s0, e0, b in runs:
                        hist.setdefault(e0 - s0, {"A": [], "T": [], "C": [], "G": []})[b].append(draws[s0])
                    inject = [list(reversed(hist[length][b])) for length in hist for b in "ATCG" if hist[length][b]]
                    calls = []

                    def normal(mu, sigma, n):
                        v = np.array(inject[len(calls)], dtype=np.float64)
                        assert len(v) == n
                        calls.append([float(x) for x in v])
                        return v

                    classes1 = [10 + (i * 7 + i // 5) % 9 for i in range(len(seq))]      # (no 1 = mis, no 2 = ins: those are the stage's own)
                    S.hp_mis_rate = rate
                    random.seed(4200 + 31 * k + (7 if long_runs else 0) + (1 if rate > 0.1 else 0))
                    np.random.normal = normal
                    try:
                        with Recorder(S) as r2:
                            out2, q2 = S.mutate_homo(seq, list(classes1), k)
                    finally:
                        np.random.normal = orig_normal
                    assert len(calls) == len(inject)
                    groups, ci = {}, 0
                    for length in hist:
                        for b in "ATCG":
                            if hist[length][b]:
                                groups[(length, b)] = list(calls[ci]); ci += 1
                    x_runs = [groups[(e0 - s0, b)].pop() for s0, e0, b in runs]          # consumed from the END (S:665-666)
                    homo.append(dict(k=k, hp_mis_rate=rate, out1=seq, classes1=classes1, x_runs=x_runs, u_homo=r2.u, out2=out2,
                                     classes2=[int(x) for x in q2], runs=[[a, b_, c] for a, b_, c in runs]))
            for variant in (0, 1):
                read, e_dict, e_count = _hp_edge_filter_case(k, variant, rng)
                random.seed(4300 + 2 * k + variant)
                log = _Log()
                with Recorder(S) as r1:
                    out1, q1 = S.mutate_read(read, "name", log, {a: list(b) for a, b in e_dict.items()}, dict(e_count), True, k)
                assert len(out1) == len(q1)
                filt.append(dict(k=k, converted=read, e_dict=edict_list(e_dict), u_mutate=r1.u, out1=out1,
                                 classes1=[int(x) for x in q1], log=log.rows))
    finally:
        S.model_base_quals.predict_base_qualities = orig_q
        S.model_hp_len.get_nd_par = orig_par
        S.hp_mis_rate = orig_rate
    return dict(homo=homo, filter=filt)


def check_hp_edges(fx):
    """the generator's guard: the oracle, replaying the fixture, must raise every branch counter the fixture is there to reach"""
    import ctypes as C
    import copy
    from nanosim_amd import model as M
    from tests import oracle_lib as O
    from tests.test_homopolymer import filter_events
    from tests.test_oracle_pin import expected_events
    L = O.lib()
    mdl = M.load_model(os.path.join(HERE, "model_small", "training"), chimeric=True, homopolymer=True, fastq=True)
    O.hp_counts()
    for case in fx["homo"]:
        m = copy.deepcopy(mdl)
        m.hp_mis_rate = case["hp_mis_rate"]
        t = m.to_c()
        d, keep = O.make_tape(case["u_homo"], z=case["x_runs"])
        seq = np.frombuffer(case["out1"].encode(), dtype=np.uint8).copy()
        q = np.array(case["classes1"], dtype=np.uint8)
        out = np.zeros(len(case["out2"]) + 64, dtype=np.uint8)
        oq = np.zeros_like(out)
        L.nso_mutate_homo(C.byref(t), seq.ctypes.data, q.ctypes.data, len(seq), case["k"], C.byref(d), 0, 0, out.ctypes.data,
                          oq.ctypes.data, len(out))
    cnt = O.hp_counts()
    missed = [c for c in HP_EDGE_HOMO_COUNTERS if not cnt[c]]
    for case in fx["filter"]:
        filter_events(L, case["converted"], expected_events(case["e_dict"]), case["k"])
    cnt2 = O.hp_counts()
    missed += [c for c in HP_EDGE_FILTER_COUNTERS if not cnt2[c]]
    assert not missed, "the fixture does not reach: %s" % ", ".join(missed)
    assert cnt["edits_max"] > 6
    return cnt, cnt2


def fixture_unaligned(S):
    """unaligned_error_list + mutate_read STRUCTURE: an all-'A' read and a choice() that never returns 'A'
    make copied bases ('A') distinguishable from generated ones."""
    cases = []
    seed = 1300
    orig_choice = random.choice
    for m_ref in (0, 3, 50, 400, 1500):
        for rep in range(4):
            random.seed(seed); np.random.seed(seed); seed += 1
            with Recorder(S) as r:
                l_new, middle_ref, e_dict, e_count = S.unaligned_error_list(m_ref, S.error_par)
            read = "A" * middle_ref

            def choice(seq):
                cand = [c for c in seq if c != "A"]
                return cand[0]

            random.choice = choice
            try:
                out, _ = S.mutate_read(read, "name", None, {a: list(b) for a, b in e_dict.items()}, dict(e_count), False, False)
            finally:
                random.choice = orig_choice
            cases.append(dict(m_ref=m_ref, u=r.u, n=r.n, l_new=int(l_new), middle_ref=int(middle_ref),
                              e_dict=edict_list(e_dict), copied_mask="".join("1" if c == "A" else "0" for c in out)))
    return cases


def fixture_samplers(S):
    """Histograms of the reference's own samplers (seeded global numpy RNG)."""
    out = {}
    n = 400000
    np.random.seed(2024)
    ep = S.error_par
    v = np.array([S.mm.pois_geom(ep["mis"][0], ep["mis"][2], ep["mis"][3]) for _ in range(n)])
    out["mis"] = np.bincount(v, minlength=64)[:64].tolist()
    for ty in ("ins", "del"):
        v = np.array([S.mm.wei_geom(ep[ty][0], ep[ty][1], ep[ty][2], ep[ty][3]) for _ in range(n)])
        out[ty] = np.bincount(v, minlength=64)[:64].tolist()
    out["n"] = n
    # qualities
    from scipy.stats import lognorm
    q = {}
    for name, par in S.lognorm_base_qual.items():
        np.random.seed(77)
        vals = np.array(S.model_base_quals.predict_base_qualities(par["sd"], par["loc"], np.exp(par["mu"]), 200000))
        fa, fb = lognorm.cdf(1, par["sd"], scale=np.exp(par["mu"])), lognorm.cdf(93, par["sd"], scale=np.exp(par["mu"]))
        ks = np.arange(1, 94)
        cdf = (lognorm.cdf(ks, par["sd"], scale=np.exp(par["mu"])) - fa) / (fb - fa)
        q[name] = dict(hist=np.bincount(vals, minlength=128)[:128].tolist(), pmf_1_92=np.diff(cdf).tolist(), par=par)
    out["quals"] = q
    # homopolymer normal parameters (get_nd_par)
    hp = {}
    for length in (5, 7, 10, 13, 20, 40):
        hp[str(length)] = [float(x) for x in S.model_hp_len.get_nd_par(length, S.pw_hp_len, S.lr_hp_len)]
    out["get_nd_par"] = hp
    out["hp_mis_rate"] = S.hp_mis_rate
    return out


def fixture_kde(S):
    out = {}
    for name, kde, log in (("aligned_region", S.kde_aligned, False), ("ht_length", S.kde_ht, True),
                           ("ht_ratio", S.kde_ht_ratio, False)):
        k = 64
        np.random.seed(31)
        x = S.get_length_kde(kde, k, log)
        np.random.seed(31)
        u = np.random.uniform(0, 1, size=k)
        g = np.random.standard_normal(k)
        data = np.asarray(kde.tree_.data)[:, 0]
        i = (u * data.shape[0]).astype(np.int64)
        x2 = data[i] + kde.bandwidth_ * g
        if log:
            x2 = np.power(10, x2) - 1
        assert np.allclose(x, x2, rtol=1e-12, atol=1e-12), name
        out[name] = dict(u=u.tolist(), g=g.tolist(), x=x.tolist(), log=log, bw=float(kde.bandwidth_))
    return out


def fixture_extract(S):
    """extract_read start positions: (randint value -> chromosome, pos) incl. rejected draws."""
    cases = []
    orig = random.randint
    for dna_type, length in (("linear", 1), ("linear", 500), ("linear", 25000), ("linear", 39990)):
        random.seed(length)
        draws = []

        def ri(a, b):
            v = orig(a, b)
            draws.append(v)
            return v

        random.randint = ri
        try:
            for _ in range(12):
                del draws[:]
                seq, name = S.extract_read(dna_type, length)
                cases.append(dict(dna_type=dna_type, length=length, draws=list(draws), name=name, seq=seq if length <= 500 else None))
        finally:
            random.randint = orig
    return dict(cases=cases, seq_len=dict(S.seq_len), genome_len=int(S.genome_len))



META_DIR = os.path.join(HERE, "meta")


def build_meta_inputs():
    """Three synthetic species (committed FASTA files + the three metagenome config files of the CLI)."""
    os.makedirs(META_DIR, exist_ok=True)
    synth.write_fasta(os.path.join(META_DIR, "Alpha_one.fa"), [("chrA1 alpha chromosome", synth.synth_sequence(120000, 301, iupac_frac=0.001))])
    synth.write_fasta(os.path.join(META_DIR, "Beta_two.fa"), [("NC_100.1 beta chromosome 1", synth.synth_sequence(90000, 302, lower_frac=0.1)),
                                                             ("NC_101.1 beta chromosome 2", synth.synth_sequence(20000, 303))])
    synth.write_fasta(os.path.join(META_DIR, "Gamma_three.fa"), [("gchr", synth.synth_sequence(60000, 304, n_frac=0.01)),
                                                                ("plasmid_p1", synth.synth_sequence(3000, 305))])
    with open(os.path.join(META_DIR, "genome_list.tsv"), "w") as f:
        f.write("Alpha one\ttests/golden/meta/Alpha_one.fa\nBeta two\ttests/golden/meta/Beta_two.fa\n"
                "Gamma three\ttests/golden/meta/Gamma_three.fa\n")
    with open(os.path.join(META_DIR, "dna_type_list.tsv"), "w") as f:
        f.write("Alpha one\tchrA1 alpha chromosome\tcircular\nBeta two\tNC_100.1 beta chromosome 1\tlinear\n"
                "Beta two\tNC_101.1 beta chromosome 2\tlinear\nGamma three\tgchr\tcircular\nGamma three\tplasmid_p1\tlinear\n")
    with open(os.path.join(META_DIR, "abundance.tsv"), "w") as f:
        f.write("Size\t3000\t500\nAlpha one\t50\t10\nBeta two\t30\t60\nGamma three\t20\t30\n")


def _meta_profile(S, prefix, chimeric, fastq=False, perfect=False):
    os.chdir(ROOT)
    so = sys.stdout
    sys.stdout = open(os.devnull, "w")
    try:
        S.read_profile(os.path.join(META_DIR, "genome_list.tsv"), [], prefix, perfect, "metagenome", None,
                       dna_type=os.path.join(META_DIR, "dna_type_list.tsv"), abun=os.path.join(META_DIR, "abundance.tsv"),
                       chimeric=chimeric, homopolymer=False, fastq=fastq)
    finally:
        sys.stdout = so


def fixture_metagenome(S, prefix):
    build_meta_inputs()
    _meta_profile(S, prefix, True)
    out = dict(species=list(S.seq_len.keys()),
               seq_len={sp: [[k, v] for k, v in S.seq_len[sp].items()] for sp in S.seq_len},
               dna_type={sp: dict(S.dict_dna_type[sp]) for sp in S.dict_dna_type},
               abun=S.multi_dict_abun, number_aligned=list(S.number_aligned_l), number_unaligned=list(S.number_unaligned_l),
               max_chrom=dict(S.max_chrom), abun_inflation=S.abun_inflation, segment_mean=S.segment_mean)
    S.dict_abun = S.multi_dict_abun["sample0"]
    S.dict_abun_inflated = {sp: S.inflate_abun(S.dict_abun, sp) for sp in S.dict_abun}
    out["abun_inflated"] = dict(S.dict_abun_inflated)
    # assign_species on tape
    cases = []
    rng = np.random.default_rng(5)
    for n_reads, chim in ((40, False), (60, True), (25, True), (300, False)):
        segs = (rng.geometric(1 / 1.6, n_reads) if chim else np.ones(n_reads, dtype=int)).tolist()
        lens = rng.lognormal(np.log(3000), 0.7, int(sum(segs))).tolist()
        if n_reads == 25:
            lens = lens[:len(lens) - 5]                      # fewer lengths than segments: the loop stops early (S:781-782)
        cur = {sp: int(rng.integers(0, 20000)) for sp in S.dict_abun}
        random.seed(n_reads)
        with Recorder(S) as r:
            sp_list, len_list, seg_arr = S.assign_species(list(lens), np.array(segs), dict(cur))
        cases.append(dict(lengths=lens, segs=segs, current=cur, u=r.u, species=list(sp_list), out_lengths=[float(x) for x in len_list],
                          out_segs=[int(x) for x in seg_arr]))
    out["assign_species"] = cases
    # extract_read("metagenome", length, species) on tape
    ex = []
    random.seed(77)
    for sp in list(S.seq_len.keys()) + [None]:
        for length in (10, 2000, 5000, 25000, 70000, 100000):
            for rep in range(3):
                with Recorder(S) as r:
                    try:
                        seq, name = S.extract_read("metagenome", length, sp)
                    except AssertionError:
                        continue
                ex.append(dict(species=sp, length=length, u=r.u, name=name, seq_len=len(seq),
                               head=seq[:30], tail=seq[-30:]))
    out["extract_read"] = ex
    # add_abundance_var on tape
    total_len = {sp: sum(S.seq_len[sp].values()) for sp in S.seq_len}
    random.seed(3)
    with Recorder(S) as r:
        av = S.add_abundance_var(S.multi_dict_abun["sample1"], total_len, -0.5, 0.5)
    out["abundance_var"] = dict(u=r.u, result=av, total_len=total_len)
    return out


def _meta_worker(args):
    idx, n_al, n_un, prefix, chimeric, workdir = args
    S = import_reference()
    _meta_profile(S, prefix, chimeric)
    S.dict_abun = S.multi_dict_abun["sample0"]
    S.dict_abun_inflated = {sp: S.inflate_abun(S.dict_abun, sp) for sp in S.dict_abun} if chimeric else {}
    S.total_simulated = mp.Value("i", 0, lock=True)
    random.seed(4000 + idx); np.random.seed(4000 + idx)
    o_reads = os.path.join(workdir, "m%d_%d.fasta" % (idx, chimeric)); o_err = os.path.join(workdir, "me%d_%d" % (idx, chimeric))
    o_un = os.path.join(workdir, "mu%d_%d.fasta" % (idx, chimeric))
    max_l = max(S.max_chrom.values())
    so = sys.stdout; se = sys.stderr
    sys.stdout = open(os.devnull, "w"); sys.stderr = open(os.devnull, "w")
    try:
        S.simulation_aligned_metagenome(50, max_l, None, None, o_reads, o_err, None, False, n_al, False, chimeric)
        S.simulation_unaligned("metagenome", 50, max_l, None, None, o_un, False, n_un, False)
    finally:
        sys.stdout = so; sys.stderr = se
    lines = open(o_reads).read().split("\n")
    names = [x[1:] for x in lines[0:-1:2]]
    lens = [len(x) for x in lines[1:-1:2]]
    species = list(S.seq_len.keys())

    def sp_of(comp):
        for sp in species:
            if comp.startswith(sp + "-"):
                return sp
        raise ValueError(comp)

    bases = {}
    n_chim = 0
    n_rev = 0
    for nm in names:
        body, _, rest = nm.partition("_aligned_")
        f = rest.split("_")
        seg_lens = [int(x) for x in f[-2].split(";")]
        comps = [c for c in body.split(";") if not c.startswith("gap_")]
        n_chim += len(comps) > 1
        n_rev += f[-4] == "R"
        for c, sl in zip(comps, seg_lens):
            bases[sp_of(c)] = bases.get(sp_of(c), 0) + sl
    strands = sorted(set(nm.partition("_aligned_")[2].split("_")[-4] for nm in names))
    un = [x[1:] for x in open(o_un).read().split("\n")[0:-1:2]]
    un_sp = {}
    for nm in un:
        un_sp[sp_of(nm)] = un_sp.get(sp_of(nm), 0) + 1
    return dict(names=names[:6], lens=lens, bases=bases, strands=strands, n_chim=n_chim, n=len(names), un_species=un_sp,
                un_names=un[:3])


def _meta_perfect_worker(args):
    idx, n_al, prefix, workdir = args
    S = import_reference()
    _meta_profile(S, prefix, False, perfect=True)
    S.dict_abun = S.multi_dict_abun["sample0"]
    S.dict_abun_inflated = {}
    S.total_simulated = mp.Value("i", 0, lock=True)
    random.seed(7000 + idx); np.random.seed(7000 + idx)
    o_reads = os.path.join(workdir, "mp%d.fasta" % idx); o_err = os.path.join(workdir, "mpe%d" % idx)
    max_l = max(S.max_chrom.values())
    so = sys.stdout; se = sys.stderr
    sys.stdout = open(os.devnull, "w"); sys.stderr = open(os.devnull, "w")
    try:
        S.simulation_aligned_metagenome(50, max_l, None, None, o_reads, o_err, None, False, n_al, True, False)
    finally:
        sys.stdout = so; sys.stderr = se
    lines = open(o_reads).read().split("\n")
    names = [x[1:] for x in lines[0:-1:2]]
    seqs = lines[1:-1:2]
    species = list(S.seq_len.keys())
    bases = {}
    for nm, sq in zip(names, seqs):
        sp = [x for x in species if nm.startswith(x + "-")][0]
        f = nm.partition("_perfect_")[2].split("_")
        assert f[2] == "0" and f[4] == "0" and int(f[3]) == len(sq)
        bases[sp] = bases.get(sp, 0) + len(sq)
    # the read is the reference substring (or its reverse complement)
    nm, sq = names[0], seqs[0]
    sp = [x for x in species if nm.startswith(x + "-")][0]
    chrom, pos = nm[len(sp) + 1:].partition("_perfect_")[0].rsplit("_", 1)
    src = S.seq_dict[sp][chrom]
    seg = (src + src)[int(pos):int(pos) + len(sq)].upper()
    strand = nm.partition("_perfect_")[2].split("_")[1]
    fwd = sq if strand == "F" else S.reverse_complement(sq)
    assert len(fwd) == len(seg) and all(a == b for a, b in zip(seg, fwd) if a in "ACGT"), "perfect read is not the reference substring"
    return dict(names=names[:5], lens=[len(x) for x in seqs], bases=bases, n=len(names),
                strands=sorted(set(n.partition("_perfect_")[2].split("_")[1] for n in names)),
                indices=[int(n.partition("_perfect_")[2].split("_")[0]) for n in names[:50]])


def fixture_metagenome_perfect(prefix, workdir, n_reads=8000):
    n_proc = min(8, os.cpu_count() or 1)
    with mp.get_context("fork").Pool(n_proc) as pool:
        res = pool.map(_meta_perfect_worker, [(i, n_reads // n_proc, prefix, workdir) for i in range(n_proc)])
    bases = {}
    for r in res:
        for sp, b in r["bases"].items():
            bases[sp] = bases.get(sp, 0) + b
    all_lens = np.concatenate([r["lens"] for r in res])
    return dict(bases=bases, q_len=quantiles(all_lens), mean_len=float(all_lens.mean()),
                workers=[dict(strands=r["strands"], n=r["n"], first_names=r["names"], indices=r["indices"],
                              sorted_desc_frac=float(np.mean(np.diff(r["lens"]) <= 0))) for r in res])


TRX_DIR = os.path.join(HERE, "trx")


def build_trx_inputs():
    os.makedirs(TRX_DIR, exist_ok=True)
    recs, expr, polya = synth.synth_transcriptome(240, 77)
    synth.write_fasta(os.path.join(TRX_DIR, "transcripts.fa"), recs)
    synth.write_expression(os.path.join(TRX_DIR, "expression.tsv"), expr)
    with open(os.path.join(TRX_DIR, "polya.txt"), "w") as f:
        f.write("\n".join(polya) + "\n")


IR_PREFIX = os.path.join(HERE, "model_small", "training")


def build_ir_inputs():
    """genome FASTA, GFF3 structure and IR Markov model for the transcripts of build_trx_inputs (synthetic, committed as data)"""
    recs, _, _ = synth.synth_transcriptome(240, 77)
    genome, gff, model = synth.synth_annotation(recs, 78)
    synth.write_fasta(os.path.join(TRX_DIR, "genome.fa"), genome)
    with open(IR_PREFIX + "_added_intron_final.gff3", "w") as f:
        f.write(gff)
    with open(IR_PREFIX + "_IR_markov_model", "w") as f:
        f.write(model)


def fixture_ir(S):
    """update_structure / ref_len_from_structure (S:100-145) pinned by value.  The structures are read with the repo's GFF3 reader
    (the reference reads them through HTSeq, which this image lacks) and handed over in the reference's tuple layout
    (type, chrom, start, end, length, strand); IR_markov_model is laid out as S:414-422 builds it.  extract_read_pos (S:148-191) runs on
    the structures update_structure returned, with random.randint on tape and HTSeq.GenomicInterval replaced by a four-field record
    (_GenomicIntervalRecord): `extract` lists, per case, the calls made (aligned length, polyA flag, uniform behind the randint) and what
    came back (intervals, retain_polya, ir_list)."""
    import random as pyrandom
    from nanosim_amd import intron_retention as IR
    structure = IR.read_structure(IR_PREFIX + "_added_intron_final.gff3")
    model = {}
    with open(IR_PREFIX + "_IR_markov_model") as f:
        f.readline()
        for line in f:
            info = line.strip().split()
            model[info[0]] = {(0, float(info[1])): "no_IR", (float(info[1]), float(info[1]) + float(info[2])): "IR"}
    rng = np.random.Generator(np.random.Philox(4242))
    tids = sorted(structure.keys())
    cases = []
    real = pyrandom.random
    real_randint = pyrandom.randint
    try:
        for ci in range(400):
            tid = tids[int(rng.integers(0, len(tids)))]
            items = structure[tid]
            n_int = sum(1 for it in items if it[0] == "intron")
            tape = [float(x) for x in rng.random(n_int)]
            if ci % 7 == 0 and n_int:                       # values on the interval borders
                tape[0] = [0.0, 0.8, 0.9, 0.6, 0.7999999999999999][ci // 7 % 5]
            it = iter(tape)
            pyrandom.random = lambda: next(it)
            flag, new = S.update_structure(items, model)
            exon_len = int(S.ref_len_from_structure(items))
            extract = []
            if flag:                                        # S:1157-1160: extract_read_pos(middle_ref, ref_trx_len, structure_new, trx_has_polya)
                len_before, ret_total = 0, sum(x[4] for x in new if x[0] == "retained_intron")
                for x in new:
                    if x[0] == "exon":
                        len_before += x[4]
                    elif x[0] == "retained_intron":
                        break
                for k in range(4):
                    length = int(rng.integers(1, exon_len + 1)) if k else exon_len          # (middle_ref <= ref_trx_len, S:1143-1144)
                    polya = bool(rng.integers(0, 2))
                    u = float(rng.random()) if (ci + k) % 5 else [0.0, 0.9999999999999999][k % 2]
                    if k == 3:                              # a read that starts late enough to reach the 3' end through the retained introns
                        s_ = min(len_before, ret_total + int(rng.integers(0, 12)) - 6, exon_len - 1)
                        if s_ < 0:
                            continue
                        length, polya, u = exon_len - s_, True, 0.9999999999999999
                    pyrandom.randint = lambda a_, b_, u=u: a_ + min(int(u * (b_ - a_ + 1)), b_ - a_)
                    ivs, retain_polya, ir_list = S.extract_read_pos(length, exon_len, new, polya)
                    extract.append(dict(length=length, polya=polya, u=u, retain_polya=bool(retain_polya),
                                        intervals=[[str(iv.chrom), int(iv.start), int(iv.end), str(iv.strand)] for iv in ivs],
                                        ir_list=[[int(a_), int(b_)] for a_, b_ in ir_list]))
            cases.append(dict(tid=tid, u=tape, flag=bool(flag), retained=[1 if x[0] == "retained_intron" else 0 for x in new if x[0] != "exon"],
                              exon_len=exon_len, extract=extract))
    finally:
        pyrandom.random = real
        pyrandom.randint = real_randint
    return dict(cases=cases)


class _FastafileStandIn:
    """What the transcriptome worker uses of pysam.Fastafile (S:1066-1070, 1164-1171): `.references` (the sequence names up to the first
    white space, in file order) and `.fetch(chrom, start, end)` = bases [start, end) of that sequence, 0-based, half open, in the case of
    the file — pysam's documented semantics.  pysam is not in the image; with this record in its place the reference's own splice
    (fetch of every interval, concatenation, reverse_complement on strand '-') runs here on the committed trx/genome.fa."""
    def __init__(self, path):
        self.seqs, name, chunks = {}, None, []
        with open(path) as f:
            for line in f:
                if line.startswith(">"):
                    if name is not None:
                        self.seqs[name] = "".join(chunks)
                    name, chunks = line[1:].split()[0], []
                else:
                    chunks.append(line.strip())
        if name is not None:
            self.seqs[name] = "".join(chunks)
        self.references = list(self.seqs.keys())

    def fetch(self, chrom, start, end):
        return self.seqs[chrom][start:end]


def fixture_ir_splice(S, prefix, n_reads=1500):
    """The intron splice of simulation_aligned_transcriptome(model_ir=True) (S:1156-1178) pinned by value: the reference's worker runs
    on the committed transcriptome + GFF3 structure + IR Markov model with `genome_fai` = _FastafileStandIn(trx/genome.fa); for every
    read that went through extract_read_pos the fixture keeps the intervals it returned and the string the worker built from them
    (what it hands to case_convert: fetches concatenated, reverse-complemented when the last interval is on strand '-') — as length,
    SHA-1 and both ends.  dict_ref_structure is read with the repo's GFF3 reader in the reference's tuple layout (HTSeq is absent)."""
    import hashlib
    from nanosim_amd import intron_retention as IR
    _trx_profile(S, prefix)
    S.dict_ref_structure = IR.read_structure(IR_PREFIX + "_added_intron_final.gff3")
    S.IR_markov_model = {}
    with open(IR_PREFIX + "_IR_markov_model") as f:                      # S:414-422
        f.readline()
        for line in f:
            info = line.strip().split()
            S.IR_markov_model[info[0]] = {(0, float(info[1])): "no_IR", (float(info[1]), float(info[1]) + float(info[2])): "IR"}
    S.genome_fai = _FastafileStandIn(os.path.join(TRX_DIR, "genome.fa"))
    S.total_simulated = mp.Value("i", 0, lock=True)
    random.seed(4711); np.random.seed(4711)
    last = {"iv": None}
    records = []
    o_erp, o_ert, o_cc = S.extract_read_pos, S.extract_read_trx, S.case_convert

    def erp(*a, **k):
        out = o_erp(*a, **k)
        last["iv"] = out
        return out

    def ert(*a, **k):
        last["iv"] = None
        return o_ert(*a, **k)

    def cc(seq):
        if last["iv"] is not None:
            ivs, retain_polya, ir_list = last["iv"]
            last["iv"] = None
            records.append(dict(intervals=[[str(iv.chrom), int(iv.start), int(iv.end), str(iv.strand)] for iv in ivs],
                                ir_list=[[int(a_), int(b_)] for a_, b_ in ir_list], length=len(seq),
                                sha1=hashlib.sha1(seq.encode()).hexdigest(), head=seq[:24], tail=seq[-24:]))
        return o_cc(seq)
    S.extract_read_pos, S.extract_read_trx, S.case_convert = erp, ert, cc
    workdir = tempfile.mkdtemp(prefix="nsgolden_ir_")
    so, se = sys.stdout, sys.stderr
    sys.stdout = open(os.devnull, "w"); sys.stderr = open(os.devnull, "w")
    try:
        S.simulation_aligned_transcriptome(True, os.path.join(workdir, "r.fasta"), os.path.join(workdir, "e"), None, "guppy", n_reads, True, False)
    finally:
        sys.stdout, sys.stderr = so, se
        S.extract_read_pos, S.extract_read_trx, S.case_convert = o_erp, o_ert, o_cc
        shutil.rmtree(workdir, ignore_errors=True)
    return dict(n_reads=n_reads, references=S.genome_fai.references, spliced=records)


def _trx_profile(S, prefix, perfect=False, fastq=False):
    so = sys.stdout
    sys.stdout = open(os.devnull, "w")
    try:
        S.read_profile("", [1000], prefix, perfect, "transcriptome", None, ref_t=os.path.join(TRX_DIR, "transcripts.fa"),
                       polya=os.path.join(TRX_DIR, "polya.txt"), exp=os.path.join(TRX_DIR, "expression.tsv"), model_ir=False,
                       fastq=fastq)
    finally:
        sys.stdout = so


def fixture_transcriptome(S, prefix):
    """make_cdf, random.choices and extract_read_trx pinned by value (S:69-97, 1084, 1683-1691)"""
    _trx_profile(S, prefix)
    fx = dict(ecdf_length_list=[[k, int(v)] for k, v in S.ecdf_length_list], ecdf_weight_list=[float(x) for x in S.ecdf_weight_list],
              seq_len={k: int(v) for k, v in list(S.seq_len.items())[:20]}, n_trx=len(S.seq_len),
              polya=sorted(S.trx_with_polya.keys())[:20], n_polya=len(S.trx_with_polya))
    us = [0.0, 1e-9, 0.013, 0.25, 0.5, 0.77, 0.9, 0.99, 0.999999, 0.37, 0.61]
    picks = []
    for u in us:                                       # random.choices calls the hidden instance's method, not the module attribute
        random._inst.random = lambda u=u: u
        try:
            picks.append(list(random.choices(S.ecdf_length_list, weights=S.ecdf_weight_list, k=1)[0]))
        finally:
            del random._inst.random
    fx["choices"] = dict(u=us, picks=[[p[0], int(p[1])] for p in picks])
    ext = []
    keys = list(S.seq_len.keys())
    S.trx_with_polya = S.trx_with_polya
    for i in range(40):
        key = keys[(i * 7) % len(keys)]
        length = max(1, S.seq_len[key] - (i * 13) % 60)
        rec = {}
        orig_ri = random.randint
        def ri(a, b, rec=rec):
            v = orig_ri(a, b)
            rec.update(a=a, b=b, v=v)
            return v
        random.randint = ri
        try:
            read, pos, retain = S.extract_read_trx(key, length, key in S.trx_with_polya)
        finally:
            random.randint = orig_ri
        ext.append(dict(key=key, length=length, randint=[rec["a"], rec["b"], rec["v"]], pos=pos, retain=bool(retain), head=read[:12]))
    fx["extract_read_trx"] = ext
    samp = np.array([[100.0, 80.2], [250.0, 200.9], [251.0, 10.5], [1000.0, 999.99], [4000.0, 3500.4]])
    fx["select_nearest"] = [[L, int(S.select_nearest_kde2d(samp, L))] for L in (1, 120, 250.4, 250.6, 2000, 2600, 9999)]
    return fx


def fixture_trx_walk(S, prefix, n_reads=4000):
    """The transcript pick walk of simulation_aligned_transcriptome (S:1080-1104) as a TAPE: the reference's worker runs with
    random.choices, get_length_kde(kde_aligned_2d) and select_nearest_kde2d wrapped, and the fixture keeps, for every pick in order,
    [index of the transcript in ecdf_length_list, the ref_len_aligned the reference looked up, 1 if a new KDE sample was drawn before the
    look-up (S:1087-1092), 1 if the pick ended the inner loop (S:1103-1104)] — plus the transcripts of the reads the worker wrote, which
    must be the accepted picks in order.  tests/test_transcriptome.py replays the picks and look-ups through the oracle's walk."""
    _trx_profile(S, prefix, perfect=True)
    S.total_simulated = mp.Value("i", 0, lock=True)
    random.seed(2718); np.random.seed(2718)
    index_of = {name: i for i, (name, _) in enumerate(S.ecdf_length_list)}
    st = {"sample": 0, "at_pick": 0}
    picks = []
    o_choices, o_glk, o_near = random.choices, S.get_length_kde, S.select_nearest_kde2d

    def choices(population, *a, **k):
        out = o_choices(population, *a, **k)
        if population is S.ecdf_length_list:
            st["at_pick"] = st["sample"]
            picks.append([index_of[out[0][0]], None, None, None])
        return out

    def glk(kde, *a, **k):
        if kde is S.kde_aligned_2d:
            st["sample"] += 1
        return o_glk(kde, *a, **k)

    def near(sampled, ref_len_total):
        y = o_near(sampled, ref_len_total)
        pk = picks[-1]
        pk[1], pk[2], pk[3] = int(y), int(st["sample"] != st["at_pick"]), int(y < ref_len_total)
        return y
    random.choices, S.get_length_kde, S.select_nearest_kde2d = choices, glk, near
    workdir = tempfile.mkdtemp(prefix="nsgolden_walk_")
    so, se = sys.stdout, sys.stderr
    sys.stdout = open(os.devnull, "w"); sys.stderr = open(os.devnull, "w")
    try:
        S.simulation_aligned_transcriptome(False, os.path.join(workdir, "r.fasta"), os.path.join(workdir, "e"), None, "guppy", n_reads, True,
                                           False, True, False)
        lines = open(os.path.join(workdir, "r.fasta")).read().split("\n")
    finally:
        sys.stdout, sys.stderr = so, se
        random.choices, S.get_length_kde, S.select_nearest_kde2d = o_choices, o_glk, o_near
        shutil.rmtree(workdir, ignore_errors=True)
    written = [index_of[x[1:].partition("_perfect_")[0].rsplit("_", 1)[0]] for x in lines[0:-1:2]]
    assert all(p[1] is not None for p in picks)
    return dict(n_reads=n_reads, n_samples=st["sample"], lengths=[int(v) for _, v in S.ecdf_length_list], picks=picks, written=written)


def _trx_worker(args):
    idx, n_al, prefix, workdir, perfect, uracil = args
    S = import_reference()
    _trx_profile(S, prefix, perfect=perfect)
    S.total_simulated = mp.Value("i", 0, lock=True)
    random.seed(9000 + idx); np.random.seed(9000 + idx)
    tag = "%d_%d_%d" % (idx, perfect, uracil)
    o_reads = os.path.join(workdir, "t%s.fasta" % tag); o_err = os.path.join(workdir, "te%s" % tag)
    so = sys.stdout; se = sys.stderr
    sys.stdout = open(os.devnull, "w"); sys.stderr = open(os.devnull, "w")
    try:
        S.simulation_aligned_transcriptome(False, o_reads, o_err, None, "guppy", n_al, True, False, perfect, uracil)
    finally:
        sys.stdout = so; sys.stderr = se
    lines = open(o_reads).read().split("\n")
    names = [x[1:] for x in lines[0:-1:2]]
    seqs = lines[1:-1:2]
    out = dict(trx=[], pos=[], head=[], mid=[], tailp=[], rev=[], seq_len=[len(x) for x in seqs], names=names[:5],
               has_t=any("T" in x for x in seqs[:200]), has_u=any("U" in x for x in seqs[:200]))
    for nm in names:
        body, _, rest = nm.partition("_perfect_" if perfect else "_aligned_")
        trx, pos = body.rsplit("_", 1)
        f = rest.split("_")
        out["trx"].append(trx); out["pos"].append(int(pos)); out["rev"].append(f[1] == "R")
        out["head"].append(int(f[2])); out["mid"].append(int(f[3])); out["tailp"].append(int(f[4]))
    out["seq_lens_of"] = {k: int(v) for k, v in S.seq_len.items()}
    out["polya_listed"] = sorted(S.trx_with_polya.keys())
    return out


def fixture_transcriptome_runs(prefix, workdir, n_reads=16000, per_worker=None, which=("aligned", "perfect"), seed_base=0):
    """per_worker: reads per reference worker (= num_simulate of S:1080: the size of the worker's 2-D KDE sample); default n_reads / 8"""
    out = {}
    n_proc = min(8, os.cpu_count() or 1)
    per_worker = per_worker or n_reads // n_proc
    n_workers = max(1, n_reads // per_worker)
    for name, perfect, uracil in (("aligned", False, False), ("perfect", True, True)):
        if name not in which:
            continue
        with mp.get_context("fork").Pool(n_proc) as pool:
            res = pool.map(_trx_worker, [(seed_base + i, per_worker, prefix, workdir, perfect, uracil) for i in range(n_workers)])
        lens = res[0]["seq_lens_of"]
        listed = set(res[0]["polya_listed"])
        trx = [t for r in res for t in r["trx"]]
        mid = np.array([m for r in res for m in r["mid"]], dtype=np.float64)
        pos = np.array([m for r in res for m in r["pos"]], dtype=np.float64)
        tl = np.array([lens[t] for t in trx], dtype=np.float64)
        tailp = np.array([m for r in res for m in r["tailp"]], dtype=np.float64)
        head = np.array([m for r in res for m in r["head"]], dtype=np.float64)
        seq_len = np.array([m for r in res for m in r["seq_len"]], dtype=np.float64)
        reach = np.array([(t in listed) and (p + m + 10 >= l) for t, p, m, l in zip(trx, pos, mid, tl)])
        counts = {}
        for t in trx:
            counts[t] = counts.get(t, 0) + 1
        out[name] = dict(n=len(trx), counts=counts, q_mid=quantiles(mid), q_frac=quantiles(mid / tl), q_start_frac=quantiles(pos / np.maximum(1, tl - mid)),
                         q_tailp=quantiles(tailp), q_head=quantiles(head), q_seq_len=quantiles(seq_len), frac_rev=float(np.mean([x for r in res for x in r["rev"]])),
                         frac_reach_end=float(reach.mean()), q_tailp_reach=quantiles(tailp[reach]) if reach.any() else [],
                         q_tailp_noreach=quantiles(tailp[~reach]), first_names=res[0]["names"], has_t=any(r["has_t"] for r in res),
                         has_u=any(r["has_u"] for r in res))
    return out


def fixture_metagenome_runs(prefix, workdir, n_reads=24000):
    out = {}
    for chim in (False, True):
        n_proc = min(8, os.cpu_count() or 1)
        args = [(i, n_reads // n_proc, 300, prefix, chim, workdir) for i in range(n_proc)]
        with mp.get_context("fork").Pool(n_proc) as pool:
            res = pool.map(_meta_worker, args)
        bases = {}
        for r in res:
            for sp, b in r["bases"].items():
                bases[sp] = bases.get(sp, 0) + b
        un = {}
        for r in res:
            for sp, b in r["un_species"].items():
                un[sp] = un.get(sp, 0) + b
        all_lens = np.concatenate([r["lens"] for r in res])
        out["chimeric" if chim else "plain"] = dict(
            bases=bases, workers=[dict(strands=r["strands"], n=r["n"], n_chim=r["n_chim"], first_names=r["names"],
                                       lens_head=r["lens"][:50], sorted_desc_frac=float(np.mean(np.diff(r["lens"]) <= 0)))
                                  for r in res],
            q_len=quantiles(all_lens), mean_len=float(all_lens.mean()), unaligned_species=un, un_names=res[0]["un_names"])
    return out

def _dist_worker(args):
    dna_type = "linear"
    if len(args) == 10:
        args, dna_type = args[:9], args[9]
    idx, n_al, n_un, prefix, fasta, workdir, fastq, kmer, chimeric = args
    S = import_reference()
    devnull = open(os.devnull, "w")
    so = sys.stdout
    sys.stdout = devnull
    try:
        S.read_profile(fasta, [n_al + n_un], prefix, False, "genome", None, dna_type=dna_type, chimeric=chimeric,
                       homopolymer=bool(kmer), fastq=fastq)
    finally:
        sys.stdout = so
    S.total_simulated = mp.Value("i", 0, lock=True)
    random.seed(1000 + idx); np.random.seed(1000 + idx)
    ext = ".fastq" if fastq else ".fasta"
    o_reads = os.path.join(workdir, "al%d%s" % (idx, ext))
    o_err = os.path.join(workdir, "err%d" % idx)
    o_un = os.path.join(workdir, "un%d%s" % (idx, ext))
    sys.stdout = devnull
    try:
        S.simulation_aligned_genome(dna_type, 50, S.max_chrom, None, None, o_reads, o_err, kmer, fastq, n_al, False, chimeric)
        S.simulation_unaligned(dna_type, 50, S.max_chrom, None, None, o_un, fastq, n_un, False)
    finally:
        sys.stdout = so
    # per-read metrics
    lens, heads, tails, refl, rev, nseg = [], [], [], [], [], []
    names = []
    qual_hist = np.zeros(128, dtype=np.int64)
    step = 4 if fastq else 2
    with open(o_reads) as f:
        lines = f.read().split("\n")
    for i in range(0, len(lines) - 1, step):
        nm = lines[i][1:]
        parts = nm.split("_")
        segl = [int(x) for x in parts[-2].split(";")]                   # chimeric: one reference length per segment (S:1399-1401)
        lens.append(len(lines[i + 1])); heads.append(int(parts[-3])); refl.append(sum(segl)); tails.append(int(parts[-1]))
        rev.append(parts[-4] == "R"); nseg.append(len(segl))
        names.append(nm)
        if fastq:
            qual_hist += np.bincount(np.frombuffer(lines[i + 3].encode(), dtype=np.uint8) - 33, minlength=128)[:128]
    cnt = {nm: [0, 0, 0, 0, 0, 0] for nm in names}
    tix = {"mis": 0, "ins": 1, "del": 2}
    with open(o_err) as f:
        for line in f:
            p = line.split("\t")
            c = cnt.get(p[0])
            if c is None:           # rows of a read that failed the final length check AFTER mutate_read had logged them (S:1429-1430 behind
                continue            # S:2006-2008): the reference leaves them in the profile; the read itself was never written
            c[tix[p[2]]] += 1
            c[3 + tix[p[2]]] += int(p[3])
    ev = np.array([cnt[nm] for nm in names], dtype=np.int64)
    ulens, urev = [], []
    with open(o_un) as f:
        lines = f.read().split("\n")
    for i in range(0, len(lines) - 1, step):
        ulens.append(len(lines[i + 1])); urev.append(lines[i].split("_")[-4] == "R")
    first = dict(aligned=names[:5], err_rows=open(o_err).read().split("\n")[:5],
                 chimeric_names=[nm for nm in names if "_chimeric_" in nm][:8])
    return dict(lens=lens, heads=heads, tails=tails, refl=refl, rev=rev, ev=ev, ulens=ulens, urev=urev,
                qual_hist=qual_hist, first=first, nseg=nseg)


def quantiles(x, k=2048):
    x = np.sort(np.asarray(x, dtype=np.float64))
    idx = ((np.arange(k) + 0.5) / k * len(x)).astype(np.int64)
    return x[idx].tolist()


def fixture_distributions(prefix, fasta, workdir, n_reads, fastq, kmer=None, chimeric=False, n_unaligned=None, dna_type="linear"):
    n_proc = min(8, os.cpu_count() or 1)
    n_al = int(round(n_reads * 19.0 / 20.0))
    n_un = n_reads - n_al if n_unaligned is None else n_unaligned
    args = [(i, n_al // n_proc, max(1, n_un // n_proc), prefix, fasta, workdir, fastq, kmer, chimeric, dna_type) for i in range(n_proc)]
    with mp.get_context("fork").Pool(n_proc) as pool:
        res = pool.map(_dist_worker, args)
    cat = lambda k: np.concatenate([np.asarray(r[k]) for r in res])
    ev = np.concatenate([r["ev"] for r in res])
    out = dict(n_aligned=int(len(cat("lens"))), n_unaligned=int(len(cat("ulens"))), fastq=fastq,
               q_len=quantiles(cat("lens")), q_head=quantiles(cat("heads")), q_tail=quantiles(cat("tails")),
               q_ref_len=quantiles(cat("refl")), rev_frac=float(cat("rev").mean()),
               q_unaligned_len=quantiles(cat("ulens")), unaligned_rev_frac=float(cat("urev").mean()),
               first=res[0]["first"])
    for j, nm in enumerate(("mis_events", "ins_events", "del_events", "mis_bases", "ins_bases", "del_bases")):
        out["q_" + nm] = quantiles(ev[:, j])
        out["mean_" + nm] = float(ev[:, j].mean())
    out["mean_len"] = float(cat("lens").mean())
    if chimeric:
        # segments per read (S:1276-1279), bases contributed by the gaps of a chimeric read (simulation_gap, S:1355-1358, 1552-1568):
        # read length - head - tail - sum(segment reference lengths) - inserted + deleted bases of the logged events
        ns = cat("nseg")
        gap = cat("lens") - cat("heads") - cat("tails") - cat("refl") - ev[:, 4] + ev[:, 5]
        out["nseg_hist"] = np.bincount(ns, minlength=16).tolist()
        out["q_gap_bases_chimeric"] = quantiles(gap[ns > 1])
        out["gap_bases_nonchimeric_max_abs"] = int(np.abs(gap[ns == 1]).max())
        out["mean_gap_bases_per_gap"] = float(gap[ns > 1].sum() / (ns[ns > 1] - 1).sum())
    if fastq:
        out["qual_hist"] = np.sum([r["qual_hist"] for r in res], axis=0).tolist()
    return out


def fixture_coverage(prefix, fasta):
    """calculate_read_number_from_coverage (S:2024-2068) is a Monte-Carlo estimate (10^7 KDE samples from the global numpy generator):
    its value for three seeds and two coverages; the build's closed form must land inside their spread."""
    S = import_reference()
    out = []
    for seed in (1, 2, 3):
        for cov in (30.0, 5000.0):
            np.random.seed(seed)
            out.append(dict(seed=seed, coverage=cov, reads=int(S.calculate_read_number_from_coverage(fasta, prefix, cov))))
    return dict(reference_fasta="genome_small.fa", cases=out)


def write_distributions(prefix, fasta, workdir, n):
    """Every run is large enough for the 1 % KS gate of the north star (noise floor of two 10^5-read samples: ~0.004)."""
    d = dict(fasta=fixture_distributions(prefix, fasta, workdir, n, False, n_unaligned=n),
             fastq=fixture_distributions(prefix, fasta, workdir, max(2000, n // 10), True),
             hp=fixture_distributions(prefix, fasta, workdir, n, True, kmer=5, n_unaligned=8),
             chimeric=fixture_distributions(prefix, fasta, workdir, n, False, chimeric=True, n_unaligned=8))
    with open(os.path.join(HERE, "reference_distributions.json"), "w") as f:
        json.dump(d, f)
    print("reference_distributions.json written")


HG002_SEED = 20260926          # bench.py's SEED: the model and the reference of the headline workload


def write_hg002(workdir, n):
    """The north-star gate on the north-star workload: the unmodified reference on the `hg002_like` model bench.py times (n_train 10^6 per
    KDE, aligned regions of 8.4 kb on average) and its `ecoli_like` reference (4 641 652 bp, circular) — n aligned + 100 000 unaligned reads.
    Neither input is committed (the tests rebuild both from nanosim_amd/synth.py by seed); the fixture is the quantile summary."""
    prefix = os.path.join(workdir, "hg002", "training")
    synth.write_model(prefix, synth.SynthModelSpec(n_train=1_000_000, seed=HG002_SEED), write_pkl=True, write_npz=False)
    fasta = os.path.join(workdir, "ecoli_like.fa")
    synth.write_fasta(fasta, [("ecoli-like", synth.synth_sequence(synth.ECOLI_LEN, HG002_SEED, n_frac=0.0005, iupac_frac=0.0002, lower_frac=0.02, hp_boost=0.005))])
    d = fixture_distributions(prefix, fasta, workdir, int(round(n * 20.0 / 19.0)), False, n_unaligned=100000, dna_type="circular")
    d["model"] = dict(spec="synth.SynthModelSpec(n_train=1_000_000, seed=%d)" % HG002_SEED,
                      reference="synth.synth_sequence(ECOLI_LEN, %d, n_frac=0.0005, iupac_frac=0.0002, lower_frac=0.02, hp_boost=0.005), circular" % HG002_SEED)
    with open(os.path.join(HERE, "reference_hg002.json"), "w") as f:
        json.dump(d, f)
    print("reference_hg002.json written: %d aligned, %d unaligned reads" % (d["n_aligned"], d["n_unaligned"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dist-reads", type=int, default=100000)
    ap.add_argument("--skip-dist", action="store_true")
    ap.add_argument("--only-meta-perfect", action="store_true", help="add runs.perfect to reference_metagenome.json, keep the rest")
    ap.add_argument("--only-trx", action="store_true", help="write reference_transcriptome.json only")
    ap.add_argument("--only-trx-sizes", action="store_true", help="write reference_transcriptome_sizes.json only: the transcriptome worker at 125, 1 000 and 50 000 reads per worker")
    ap.add_argument("--only-ir", action="store_true", help="write the intron-retention inputs and reference_ir.json only")
    ap.add_argument("--only-ir-splice", action="store_true", help="write reference_ir_splice.json only (the intron splice of the transcriptome worker)")
    ap.add_argument("--only-trx-walk", action="store_true", help="write reference_trx_walk.json only (the pick walk of the transcriptome worker as a tape)")
    ap.add_argument("--only-chimeric-sparse", action="store_true",
                    help="write reference_chimeric_sparse.json only: genome mode --chimeric with the committed small model AS IT IS (1.05 segments "
                         "per read, the share of the bench model) on --dist-reads reads — at 1 450 000 the fixture holds > 6 x 10^4 chimeric reads, "
                         "enough for the 1 %% gate on the gap lengths that the 114 000-read run of reference_distributions.json cannot carry")
    ap.add_argument("--only-chimeric-dense", action="store_true",
                    help="write reference_chimeric_dense.json only: genome mode --chimeric with the small model at 2 segments per read on average, "
                         "so that the fixture holds > 10^5 chimeric reads (gap lengths and segment counts at the 1 %% gate)")
    ap.add_argument("--only-dist", action="store_true", help="write reference_distributions.json only (whole-run distribution pins)")
    ap.add_argument("--only-hg002", action="store_true", help="write reference_hg002.json only: the bench-scale model (n_train 10^6, mean 8.4 kb) on the ecoli_like reference, --dist-reads aligned reads")
    ap.add_argument("--only-coverage", action="store_true", help="write reference_coverage.json only (-x / --coverage read counts)")
    ap.add_argument("--only-meta-runs", action="store_true", help="replace the whole-run part (runs) of reference_metagenome.json: 8 workers x 12 500 reads, plain and chimeric, + 8 x 6 000 perfect reads")
    ap.add_argument("--only-hp-edges", action="store_true", help="write reference_hp_edges.json.gz only (-k: hand-built inputs and injected draws at the branches the sampled tapes do not reach)")
    a = ap.parse_args()
    workdir = tempfile.mkdtemp(prefix="nsgolden_")
    try:
        if a.only_ir:
            build_ir_inputs()
            with open(os.path.join(HERE, "reference_ir.json"), "w") as f:
                json.dump(fixture_ir(import_reference()), f)
            print("reference_ir.json written")
            return
        if a.only_hg002:
            write_hg002(workdir, a.dist_reads)
            return
        prefix, fasta, circ = build_inputs(workdir)
        if a.only_hp_edges:
            import gzip
            S = import_reference()
            so = sys.stdout
            sys.stdout = open(os.devnull, "w")
            try:
                S.read_profile(fasta, [1000], prefix, False, "genome", None, dna_type="linear", chimeric=True, homopolymer=True, fastq=True)
            finally:
                sys.stdout = so
            fx = fixture_hp_edges(S)
            cnt, cnt2 = check_hp_edges(fx)                    # a fixture that misses a branch is not written
            path = os.path.join(HERE, "reference_hp_edges.json.gz")
            with gzip.GzipFile(path, "wb", mtime=0) as f:
                f.write(json.dumps(fx, separators=(",", ":")).encode())
            print("reference_hp_edges.json.gz written:", len(fx["homo"]), "mutate_homo cases,", len(fx["filter"]), "filter cases,",
                  os.path.getsize(path), "bytes")
            print("counters (mutate_homo):", cnt)
            print("counters (filter):", cnt2)
            return
        if a.only_ir_splice:
            with open(os.path.join(HERE, "reference_ir_splice.json"), "w") as f:
                json.dump(fixture_ir_splice(import_reference(), prefix), f)
            print("reference_ir_splice.json written")
            return
        if a.only_trx_walk:
            build_trx_inputs()
            fx = fixture_trx_walk(import_reference(), prefix)
            with open(os.path.join(HERE, "reference_trx_walk.json"), "w") as f:
                json.dump(fx, f, separators=(",", ":"))
            print("reference_trx_walk.json written:", len(fx["picks"]), "picks,", fx["n_samples"], "KDE samples,", len(fx["written"]), "reads")
            return
        if a.only_chimeric_sparse:
            fx = fixture_distributions(prefix, fasta, workdir, a.dist_reads, False, chimeric=True, n_unaligned=8)
            with open(os.path.join(HERE, "reference_chimeric_sparse.json"), "w") as f:
                json.dump(fx, f)
            print("reference_chimeric_sparse.json written:", fx["n_aligned"], "aligned reads,", sum(fx["nseg_hist"][2:]), "chimeric")
            return
        if a.only_chimeric_dense:
            spec = synth.SynthModelSpec(**SMALL_SPEC, segment_mean=CHIMERIC_DENSE_MEAN)       # the committed small model but for _chimeric_info
            prefix2 = os.path.join(workdir, "model_dense", "training")
            synth.write_model(prefix2, spec, write_pkl=True, write_npz=False)
            fx = fixture_distributions(prefix2, fasta, workdir, a.dist_reads, False, chimeric=True, n_unaligned=8)
            fx["segment_mean"] = CHIMERIC_DENSE_MEAN
            with open(os.path.join(HERE, "reference_chimeric_dense.json"), "w") as f:
                json.dump(fx, f)
            print("reference_chimeric_dense.json written:", fx["n_aligned"], "aligned reads,", sum(fx["nseg_hist"][2:]), "chimeric")
            return
        if a.only_trx_sizes:
            # the sample-until-repeat rule of S:1080-1104 at worker sizes well away from the 12 000 of reference_transcriptome.json: the
            # reference's worker keeps a sample of num_simulate = (reads of the worker) points, the restatement one of unbounded size per
            # block of 1 024 read indices.  Same committed inputs; 768 workers x 125 reads, 96 x 1 000 (aligned and --perfect) and 8 x 50 000.
            build_trx_inputs()
            fx = {}
            for tag, n, per, which, sb in (("w125", 96000, 125, ("aligned",), 1000), ("w1000", 96000, 1000, ("aligned", "perfect"), 2000),
                                           ("w50000", 400000, 50000, ("aligned",), 300)):
                runs = fixture_transcriptome_runs(prefix, workdir, n_reads=n, per_worker=per, which=which, seed_base=sb)
                for name, r in runs.items():
                    r["per_worker"] = per
                    fx["%s_%s" % (tag, name)] = r
                print(tag, "done", flush=True)
            with open(os.path.join(HERE, "reference_transcriptome_sizes.json"), "w") as f:
                json.dump(fx, f)
            print("reference_transcriptome_sizes.json written")
            return
        if a.only_trx:
            build_trx_inputs()
            fx = fixture_transcriptome(import_reference(), prefix)
            fx["runs"] = fixture_transcriptome_runs(prefix, workdir, n_reads=96000)
            with open(os.path.join(HERE, "reference_transcriptome.json"), "w") as f:
                json.dump(fx, f)
            print("reference_transcriptome.json written")
            return
        if a.only_dist:
            write_distributions(prefix, fasta, workdir, a.dist_reads)
            return

        if a.only_meta_runs:
            mg = json.load(open(os.path.join(HERE, "reference_metagenome.json")))
            mg["runs"] = fixture_metagenome_runs(prefix, workdir, n_reads=100000)
            mg["runs"]["perfect"] = fixture_metagenome_perfect(prefix, workdir, n_reads=48000)
            mg["runs"]["reads_per_worker"] = dict(plain=12500, chimeric=12500, perfect=6000)
            with open(os.path.join(HERE, "reference_metagenome.json"), "w") as f:
                json.dump(mg, f)
            print("reference_metagenome.json: runs rewritten")
            return
        if a.only_coverage:
            with open(os.path.join(HERE, "reference_coverage.json"), "w") as f:
                json.dump(fixture_coverage(prefix, fasta), f)
            print("reference_coverage.json written")
            return
        if a.only_meta_perfect:
            mg = json.load(open(os.path.join(HERE, "reference_metagenome.json")))
            mg["runs"]["perfect"] = fixture_metagenome_perfect(prefix, workdir)
            with open(os.path.join(HERE, "reference_metagenome.json"), "w") as f:
                json.dump(mg, f)
            print("runs.perfect written")
            return
        S = import_reference()
        so = sys.stdout
        sys.stdout = open(os.devnull, "w")
        try:
            S.read_profile(fasta, [1000], prefix, False, "genome", None, dna_type="linear", chimeric=True,
                           homopolymer=True, fastq=True)
        finally:
            sys.stdout = so
        genome = "".join(S.seq_dict.values())
        fx = dict(
            ecdf=fixture_ecdf(S, prefix),
            error_list=fixture_error_list(S),
            mutate_read=fixture_mutate_read(S, genome),
            mutate_fastq_classes=fixture_mutate_fastq_classes(S, genome),
            unaligned=fixture_unaligned(S),
            kde=fixture_kde(S),
            extract=fixture_extract(S),
            names=dict(seq_names=list(S.seq_dict.keys())),
            homopolymer=fixture_homopolymer(S, genome),
        )
        with open(os.path.join(HERE, "reference_functions.json"), "w") as f:
            json.dump(fx, f)
        with open(os.path.join(HERE, "reference_samplers.json"), "w") as f:
            json.dump(fixture_samplers(S), f)
        mg = fixture_metagenome(import_reference(), prefix)
        if not a.skip_dist:
            mg["runs"] = fixture_metagenome_runs(prefix, workdir)
            mg["runs"]["perfect"] = fixture_metagenome_perfect(prefix, workdir)
        elif os.path.exists(os.path.join(HERE, "reference_metagenome.json")):
            mg["runs"] = json.load(open(os.path.join(HERE, "reference_metagenome.json"))).get("runs")
        with open(os.path.join(HERE, "reference_metagenome.json"), "w") as f:
            json.dump(mg, f)
        if not a.skip_dist:
            write_distributions(prefix, fasta, workdir, a.dist_reads)
    finally:
        shutil.rmtree(workdir, ignore_errors=True)
    print("golden fixtures written to", HERE)


if __name__ == "__main__":
    main()
