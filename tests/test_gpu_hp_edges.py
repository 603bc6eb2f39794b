"""Whole batches at the branches of the -k homopolymer stage that the trained model never reaches: homopolymer
models that grow every run many times over (several insertions at one position, the slow tiles of the final record pass), re-sample runs
to size 0 (split deletions, adjacent re-sampled runs), mismatch four bases in ten, or draw every length exactly on a tie; on a reference
made of runs of 4 .. 4200 bases, circular (reads across the origin) and as two linear chromosomes (segment ends cut runs).

Every case runs through the oracle on the CPU first (test_hp_edge_cases_on_the_oracle, in every CPU run): it must reach its branches,
counted by the oracle's branch counters (nso_hp_counts), and produce all its reads.  The gpu half then holds the engine against the
oracle with test_gpu_parity.compare.

What the oracle's branch counters (tests/oracle_lib.py HP_COUNTERS) see: "before" = the -k cases of test_gpu_parity.py
(test_gpu_equals_oracle, test_homopolymer_stage_at_every_k) run through the oracle, "tapes" = the replay of
tests/golden/reference_hp_edges.json.gz (tests/test_homopolymer.py), "batches" = the cases of this file (edits_max is a maximum):

    counter            before   tapes  batches
    runs              1012573     582   146891
    grow                92595     247    25632
    grow_15                 0     114    19794
    shrink              96723     265    62076
    shrink_4095             0       7       17
    size0                   0      84     7850
    l64                     0      70    11011
    l1024                   0      14     5669
    l4096                   0       7     1175
    at_start              235      21     1779
    at_end                263      21     1761
    mis2                 6064     248    44572
    mis_appended         2784     133    16114
    mis_mid_ins            11      23     5256
    edits3               2367     247    33121
    edits_max               6     541     1568
    tie                     0     173    54243
    adjacent           120395      42     9379
    drop_mis            56214      75   219286
    drop_ins            35460      71   114796
    drop_del            43758      78   164187
    keep_mis           594915      33   124282
    keep_ins           296096      29    62588
    keep_del           442337      36    91616
    ins_key_before       5730      14      910
    ins_key_beyond       2724      14      453
    near_end             5878      33     2509
    run_cut                85      14       22
    shift_range             0       0       27
"""
import copy
import os

import numpy as np
import pytest

from nanosim_amd import engine as E
from nanosim_amd import metagenome as MG
from nanosim_amd import model as M
from nanosim_amd import transcriptome as T
from tests import oracle_lib as O
from tests.test_gpu_parity import compare

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
META = os.path.join(GOLDEN, "meta")
TRX = os.path.join(GOLDEN, "trx")
PREFIX = os.path.join(GOLDEN, "model_small", "training")
SEED = 0x5EED4B9A11

RUN_LENGTHS = (4, 5, 6, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100, 1023, 1024, 1025, 2100, 4096, 4200)


def runs_sequence(split=False):
    """The runs reference: runs of RUN_LENGTHS bases, three times over, separated by 1 .. 39 random bases; every fourth gap is a single
    IUPAC code, every fourth has a lower-case base next to the run behind it (within k - 1 of a run at every k).  About 43 kb.
    split: the two linear chromosomes — cut inside the second copy's 2100-base run; the first starts and the second ends with a run."""
    rng = np.random.default_rng(20261018)
    out, cut, j = [], None, 0
    for rep in range(3):
        for n in RUN_LENGTHS:
            b = "ACGT"[j % 4]
            if rep == 1 and n == 2100:
                cut = sum(len(x) for x in out) + 1000
            out.append(b * n)
            nxt = "ACGT"[(j + 1) % 4]
            if j % 4 == 1:
                gap = "RYKMSWN"[(j // 4) % 7]
            else:
                g = int(rng.integers(1, 40))
                gap = ""
                while len(gap) < g:                      # random, but no three equal bases in a row; neither end lengthens a run
                    c = "ACGT"[int(rng.integers(0, 4))]
                    if (len(gap) >= 2 and gap[-1] == gap[-2] == c) or (not gap and c == b) or (len(gap) == g - 1 and c == nxt):
                        continue
                    gap += c
                if j % 4 == 3:
                    gap = gap[:-1] + gap[-1].lower()
            if not (rep == 2 and n == RUN_LENGTHS[-1]):
                out.append(gap)
            j += 1
    seq = "".join(out)
    return (seq[:cut], seq[cut:]) if split else seq


def _as_ref(names, seqs, dna_type):
    return M.make_reference(names, [np.frombuffer(s.encode(), dtype=np.uint8).copy() for s in seqs], dna_type)


def _hp_model(base, rate=None, **par):
    """deepcopy of `base` with the homopolymer length model replaced (no breakpoints) and / or its mismatch rate"""
    m = copy.deepcopy(base)
    if par:
        for cls in ("AT", "CG"):
            m.hp[cls] = dict(betas=[], breakpoints=[], const=par["const"], alpha1=par["alpha1"], intercept=par["intercept"], slope=par["slope"])
    if rate is not None:
        m.hp_mis_rate = rate
    return m


HP_MODELS = dict(
    grow=dict(const=20.0, alpha1=2.0, intercept=0.5, slope=0.05),          # several insertions per run, stacked at one offset
    vanish=dict(const=-3.0, alpha1=0.2, intercept=0.5, slope=0.1),   # size 0, split deletions, adjacent re-sampled runs
    mis=dict(rate=0.4),                                                    # the model's lengths, four mismatches in ten bases
    half=dict(const=-0.5, alpha1=1.0, intercept=0.0, slope=0.0),           # every draw exactly L - 1/2
    grow_mild=dict(const=18.0, alpha1=1.0, intercept=0.5, slope=0.05),     # metagenome: the stage's final length decides a pass's acceptance
    grow_shift=dict(const=20.0, alpha1=6.0, intercept=0.5, slope=0.05),    # a piece gains more than the shift field of an event holds
)

FILTER = ["drop_mis", "drop_ins", "drop_del", "keep_mis", "keep_ins", "keep_del"]
# what a model is there to reach, on any reference / on the runs reference
REACH = dict(grow=["grow", "grow_15", "edits3", "mis_appended", "mis_mid_ins"], vanish=["shrink", "size0", "adjacent"],
             mis=["mis2", "mis_appended", "edits3"], half=["tie", "shrink"], grow_mild=["grow_15"], grow_shift=["shift_range"])
REACH_RUNS = dict(grow=["l64", "l1024", "l4096"], vanish=["l64", "l1024", "l4096", "shrink_4095"], mis=["l64", "l1024"], half=["l64", "l1024", "l4096"])


def _cases():
    out = []
    for mname in ("grow", "vanish", "mis", "half"):
        for rname in ("small", "runs_circ"):
            reach = REACH[mname] + (REACH_RUNS[mname] if rname != "small" else []) + FILTER + ["ins_key_before", "ins_key_beyond"]
            out.append(("%s-%s-k5" % (mname, rname), "genome", rname, mname,
                        dict(n_reads=150, kmer_bias=5, fastq=True, emit_errlog=True), reach))
    for mname, rname in (("grow", "runs_circ"), ("vanish", "runs_circ"), ("mis", "small"), ("half", "small")):
        out.append(("%s-%s-k3-chimeric" % (mname, rname), "genome", rname, mname, dict(n_reads=100, kmer_bias=3, chimeric=True),
                    REACH[mname] + FILTER))
    for k in (8, 9, 16, 17):
        for mname in ("grow", "vanish"):
            out.append(("%s-runs_linear-k%d" % (mname, k), "genome", "runs_linear", mname, dict(n_reads=100, kmer_bias=k, fastq=(k % 2 == 0)),
                        # (a read's end within k - 1 of a run's end, with an event on it: only the larger k get there in 100 reads)
                        REACH[mname] + REACH_RUNS[mname] + ["at_start", "at_end", "near_end"] + (["run_cut"] if k >= 16 else [])))
    out.append(("meta-mis-k5", "meta", "meta", "mis", dict(n_reads=150, kmer_bias=5, fastq=True), REACH["mis"] + FILTER))
    out.append(("meta-grow_mild-k5", "meta", "meta", "grow_mild", dict(n_reads=150, kmer_bias=5, min_len=200, max_len=12000), REACH["grow_mild"]))
    out.append(("trx-mis-k5", "trx", "trx", "mis", dict(n_reads=150, kmer_bias=5, fastq=True, emit_errlog=True), REACH["mis"] + FILTER))
    # the shift field of the homopolymer edits: pieces of ~20 kb that gain six times their runs
    out.append(("grow_shift-runs_circ-k5", "genome", "runs_circ", "grow_shift",
                dict(n_reads=50, kmer_bias=5, median_len=20000, sd_len=0.5, max_len=10 ** 6), REACH["grow_shift"] + ["l4096"]))
    return out


CASES = _cases()


@pytest.fixture(scope="module")
def models(small_model):
    trx = M.load_model(PREFIX, transcriptome=True, fastq=True, homopolymer=True)
    out = {}
    for name, par in HP_MODELS.items():
        out[name] = _hp_model(small_model, **par)
        out["trx-" + name] = _hp_model(trx, **par)
    return out


@pytest.fixture(scope="module")
def refs(small_ref, small_model):
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        meta = MG.read_metagenome(os.path.join(META, "genome_list.tsv"), os.path.join(META, "dna_type_list.tsv"))
    finally:
        os.chdir(cwd)
    _, samples = MG.read_abundance(os.path.join(META, "abundance.tsv"), meta.species)
    trx = T.read_transcriptome(os.path.join(TRX, "transcripts.fa"), os.path.join(TRX, "expression.tsv"), os.path.join(TRX, "polya.txt"), "guppy")
    return dict(small=small_ref, runs_circ=_as_ref(["runs"], [runs_sequence()], "circular"),
                runs_linear=_as_ref(["runs-a", "runs-b"], list(runs_sequence(split=True)), "linear"), meta=meta, abun=samples[0], trx=trx)


def _params(mode, rname, case, refs):
    if mode == "trx":
        kw = dict(seed=SEED, first_read=0, max_len=10 ** 9, trx=True)
    elif mode == "meta":
        kw = dict(seed=SEED, first_read=0, max_len=int(refs["meta"].max_chrom), meta=True)
    else:
        kw = dict(seed=SEED, first_read=0, max_len=int(refs[rname].max_chrom))
    kw.update(case)
    return E.make_params(**kw)


_ORACLE = {}


def oracle_case(cid, mode, rname, mname, case, models, refs):
    """(params, oracle batch, branch counts, range redraws) of one case, computed once for both halves"""
    if cid not in _ORACLE:
        p = _params(mode, rname, case, refs)
        L = O.lib()
        O.hp_counts()
        L.nso_range_redraw_count(1)
        # (a read of the grow models is several times its reference stretch: buffers for 200 000 bytes per read)
        if mode == "meta":
            exp = O.generate_meta(models[mname], refs["meta"], refs["abun"], None, p, bytes_per_read=200000)
        elif mode == "trx":
            exp = O.generate_trx(models["trx-" + mname], refs["trx"], p, bytes_per_read=200000)
        else:
            exp = O.generate(models[mname], refs[rname], p, bytes_per_read=700000 if mname == "grow_shift" else 200000, events_per_read=8000,
                             errlog_per_read=400000)
        _ORACLE[cid] = (p, exp, O.hp_counts(), int(L.nso_range_redraw_count(1)))
    return _ORACLE[cid]


@pytest.mark.parametrize("cid,mode,rname,mname,case,reach", CASES, ids=[c[0] for c in CASES])
def test_hp_edge_cases_on_the_oracle(models, refs, cid, mode, rname, mname, case, reach):
    """every case reaches the branches it exists for on the oracle, and all its reads are produced"""
    p, exp, cnt, redraws = oracle_case(cid, mode, rname, mname, case, models, refs)
    for name in reach:
        assert cnt[name] > 0, "case %s does not reach branch %s (counts %s)" % (cid, name, cnt)
    if mname == "grow":
        assert cnt["edits_max"] > 6, "case %s: no run with more than 6 edits" % cid
    assert len(exp["reads"]) == p.n_reads and int(exp["reads"]["seq_len"].min()) > 0
    if mname == "grow_shift":
        assert redraws >= cnt["shift_range"] > 0
    else:
        assert cnt["shift_range"] == 0


def test_runs_reference_holds_its_runs(refs):
    seq = runs_sequence()
    assert 42000 < len(seq) < 45000
    import re
    found = sorted(len(m.group()) for m in re.finditer(r"A{4,}|C{4,}|G{4,}|T{4,}", seq.upper()))
    assert found == sorted(RUN_LENGTHS * 3)
    a, b = runs_sequence(split=True)
    assert a + b == seq and a[-1] == b[0] and a[0] == a[1] and b[-1] == b[-2]          # the cut lies inside a run; runs at both outer ends
    assert any(c in seq for c in "RYKMSWN") and any(c.islower() for c in seq)


@pytest.fixture(scope="module")
def engines(refs, small_model):
    made = {}

    def get(mode, rname):
        key = rname
        if key not in made:
            e = E.Engine(0)
            if mode == "meta":
                e.set_metagenome(refs["meta"], refs["abun"], None)
            elif mode == "trx":
                e.set_transcriptome(refs["trx"])
            else:
                e.set_reference(refs[rname])
            made[key] = e
        return made[key]
    yield get
    for e in made.values():
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cid,mode,rname,mname,case,reach", CASES, ids=[c[0] for c in CASES])
def test_gpu_hp_edges_equal_oracle(engines, models, refs, cid, mode, rname, mname, case, reach):
    p, exp, cnt, redraws = oracle_case(cid, mode, rname, mname, case, models, refs)
    for name in reach:
        assert cnt[name] > 0, (cid, name)
    eng = engines(mode, rname)
    eng.load_model(models[("trx-" if mode == "trx" else "") + mname])
    b = eng.generate(p)
    compare(b, exp, p)
    assert int(b.info.n_range_redraws) == redraws
    if mode == "trx":
        assert np.array_equal(b.polya(), exp["polya"])
