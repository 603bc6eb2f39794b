"""Whole batches at the parameters that reach the edges of the length draws: -med 50 -sd 20 (lognormal lengths up
to ns_exp's 1e304), -med 200000 -sd 4 (most draws above max_len), and a head/tail KDE with a heavy upper tail (pow10m1 of 2^31 and more,
up to 1e30).  Genome aligned, unaligned and --perfect, and metagenome aligned (k_meta_draw, k_meta_round).

Every case runs through the oracle on the CPU first (test_extreme_cases_on_the_oracle, in every CPU run): it must reach its edge, counted
by the oracle's edge counters (nso_edge_counts), and its largest accepted piece is bounded by max_len.  The planned pieces are bounded by
construction: aligned segments by the max_len filter, unaligned lengths above max_len are no valid draw (-1, never walked), remainders
saturate at 0x3fffffff and fail max_len.  The gpu half then holds the engine against the oracle with test_gpu_parity.compare."""
import os

import numpy as np
import pytest

from nanosim_amd import engine as E
from nanosim_amd import metagenome as MG
from nanosim_amd import model as M
from nanosim_amd.model import NS_KDE_HT
from tests import oracle_lib as O
from tests.test_gpu_parity import compare

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
META = os.path.join(GOLDEN, "meta")
EDGE_ULEN_LONG, EDGE_ULEN_HUGE, EDGE_REM_SAT, EDGE_REM_HUGE, EDGE_LEN_HUGE = range(5)
SEED = 0x5EED0E0D6E

# (id, mode, model, params, the edges the case must reach)
CASES = [
    ("genome-aligned-sd20", "genome", "small", dict(n_reads=3000, median_len=50, sd_len=20), [EDGE_LEN_HUGE]),
    ("genome-unaligned-sd20", "genome", "small", dict(n_reads=600, kind=E.NS_KIND_UNALIGNED, median_len=50, sd_len=20),
     [EDGE_ULEN_LONG, EDGE_ULEN_HUGE]),
    ("genome-perfect-sd20", "genome", "perfect", dict(n_reads=3000, kind=E.NS_KIND_PERFECT, median_len=50, sd_len=20), [EDGE_LEN_HUGE]),
    ("genome-aligned-med200k", "genome", "small", dict(n_reads=400, median_len=200000, sd_len=4, fastq=True), [EDGE_LEN_HUGE]),
    ("genome-unaligned-med200k", "genome", "small", dict(n_reads=400, kind=E.NS_KIND_UNALIGNED, median_len=200000, sd_len=4),
     [EDGE_ULEN_LONG, EDGE_ULEN_HUGE]),
    ("genome-perfect-med200k", "genome", "perfect", dict(n_reads=400, kind=E.NS_KIND_PERFECT, median_len=200000, sd_len=4),
     [EDGE_LEN_HUGE]),
    ("meta-aligned-sd20", "meta", "small", dict(n_reads=2000, median_len=50, sd_len=20, emit_errlog=True), [EDGE_LEN_HUGE]),
    ("meta-aligned-med200k", "meta", "small", dict(n_reads=400, median_len=200000, sd_len=4), [EDGE_LEN_HUGE]),
    ("genome-aligned-heavy-ht", "genome", "heavy_ht", dict(n_reads=4000, emit_errlog=True), [EDGE_REM_HUGE, EDGE_REM_SAT]),
    ("genome-aligned-heavy-ht-sd", "genome", "heavy_ht", dict(n_reads=2000, chimeric=True, median_len=3000, sd_len=1), [EDGE_REM_HUGE]),
    ("meta-aligned-heavy-ht", "meta", "heavy_ht", dict(n_reads=3000, fastq=True), [EDGE_REM_HUGE, EDGE_REM_SAT]),
]


def _heavy_ht(m):
    """the head/tail KDE (log10 of the unaligned ends) with a heavy upper tail: 3 % of its points at log10 9.4 .. 30, so pow10m1 draws
    2^31 .. 1e30 (a plain (int32_t) of them was INT32_MIN on x86 and INT32_MAX on gfx950)"""
    data, bw = m.kde[NS_KDE_HT]
    data = np.asarray(data, dtype=np.float64)
    k = max(8, len(data) * 3 // 100)
    heavy = np.linspace(9.4, 30.0, k)
    m.kde[NS_KDE_HT] = (np.ascontiguousarray(np.concatenate([data, heavy])), bw)
    return m


@pytest.fixture(scope="module")
def models():
    prefix = os.path.join(GOLDEN, "model_small", "training")
    return dict(small=M.load_model(prefix, chimeric=True, fastq=True),
                perfect=M.load_model(prefix, perfect=True, fastq=True),
                heavy_ht=_heavy_ht(M.load_model(prefix, chimeric=True, fastq=True)))


@pytest.fixture(scope="module")
def refs():
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        meta = MG.read_metagenome(os.path.join(META, "genome_list.tsv"), os.path.join(META, "dna_type_list.tsv"))
    finally:
        os.chdir(cwd)
    _, samples = MG.read_abundance(os.path.join(META, "abundance.tsv"), meta.species)
    abun = samples[0]
    return dict(genome=M.read_fasta(os.path.join(GOLDEN, "genome_small.fa"), "linear"), meta=meta, abun=abun)


def _params(mode, case, refs):
    r = refs["meta"] if mode == "meta" else refs["genome"]
    kw = dict(seed=SEED, first_read=0, max_len=int(r.max_chrom), meta=(mode == "meta"))
    kw.update(case)
    return E.make_params(**kw)


def _oracle(mode, mdl, refs, p):
    """(oracle batch, edge counts) of one case"""
    L = O.lib()
    L.nso_edge_counts(None, 1)
    if mode == "meta":
        infl = {sp: MG.inflate_abun(refs["abun"], sp, mdl.abun_inflation) for sp in refs["abun"]} if p.chimeric else None
        exp = O.generate_meta(mdl, refs["meta"], refs["abun"], infl, p)
    else:
        # (sizes_for_model would size for the heavy tail's 1e30; the accepted reads are bounded by max_len)
        # long reads: -med 200 000, and unaligned reads at -sd 20 (log-uniform up to max_len, one event per two bases)
        long = p.median_len > 10000 or (p.kind == E.NS_KIND_UNALIGNED and p.sd_len > 5)
        exp = O.generate(mdl, refs["genome"], p, bytes_per_read=120000 if long else 40000, events_per_read=30000 if long else 4000)
    cnt = np.zeros(8, dtype=np.uint64)
    L.nso_edge_counts(cnt.ctypes.data, 1)
    return exp, cnt


_ORACLE = {}


def oracle_case(cid, mode, mname, case, models, refs):
    if cid not in _ORACLE:
        p = _params(mode, case, refs)
        _ORACLE[cid] = (p,) + _oracle(mode, models[mname], refs, p)
    return _ORACLE[cid]


@pytest.mark.parametrize("cid,mode,mname,case,edges", CASES, ids=[c[0] for c in CASES])
def test_extreme_cases_on_the_oracle(models, refs, cid, mode, mname, case, edges):
    """every case reaches its edge on the oracle, and what it accepts stays within max_len (the cost check before any GPU run)"""
    p, exp, cnt = oracle_case(cid, mode, mname, case, models, refs)
    for e in edges:
        assert cnt[e] > 0, "case %s does not reach edge %d (counts %s)" % (cid, e, cnt.tolist())
    reads = exp["reads"]
    assert len(reads) == p.n_reads
    pieces = exp["pieces"]
    assert len(pieces) and int(pieces["ref_len"].max()) <= int(p.max_len)
    assert int(reads["seq_len"].max()) <= int(p.max_len) and int(reads["seq_len"].min()) >= int(p.min_len)


@pytest.fixture(scope="module")
def engines(models, refs):
    g = E.Engine(0)
    g.set_reference(refs["genome"])
    m = E.Engine(0)
    abun = refs["abun"]
    m.set_metagenome(refs["meta"], abun, {sp: MG.inflate_abun(abun, sp, models["small"].abun_inflation) for sp in abun})
    yield dict(genome=g, meta=m)
    g.close()
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cid,mode,mname,case,edges", CASES, ids=[c[0] for c in CASES])
def test_gpu_extremes_equal_oracle(engines, models, refs, cid, mode, mname, case, edges):
    p, exp, cnt = oracle_case(cid, mode, mname, case, models, refs)
    for e in edges:
        assert cnt[e] > 0, (cid, e)
    eng = engines[mode]
    eng.load_model(models[mname])
    b = eng.generate(p)
    compare(b, exp, p)
