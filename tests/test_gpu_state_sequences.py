"""Sequences of worker calls on ONE long-lived engine per mode: what a call leaves in the context (grow-only buffers on recycled memory,
the step companion's borrowed tables, the metagenome / transcriptome state, the state after a call that failed) must not change what the
next call computes.  The suite's form of the builder-run sweeps (scripts/stress_sequences*.py), trimmed to its time budget: one fixed
list of calls per mode, drawn once from a seeded generator.

Every call of up to ORACLE_MAX reads is checked against the CPU oracle (compare(): events, pieces, records, error profile, events_used;
metagenome: the per-species bases).  A larger call is checked against the same call on a FRESH engine (records, error profile, per-read
structs, species bases) and, in genome and transcriptome mode, 64 seeded sample reads of it against the oracle (a read is a function
of (seed, read index) there; a metagenome read also depends on the passes of its batch, so its big calls have the fresh-engine check).
At most two engines are open at a time."""
import os

import numpy as np
import pytest

from nanosim_amd import engine as E
from nanosim_amd import intron_retention as IR
from nanosim_amd import metagenome as MG
from nanosim_amd import model as M
from nanosim_amd import transcriptome as T
from tests import oracle_lib as O
from tests.test_gpu_parity import compare

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PREFIX = os.path.join(GOLDEN, "model_small", "training")
META = os.path.join(GOLDEN, "meta")
TRX = os.path.join(GOLDEN, "trx")
ORACLE_MAX = 4095
SEED = 0x5E0_0E5E
BIG_FIRST = (1 << 33) + 17                      # read numbers beyond 2^32


def _flags(rng, kinds):
    """the options of one call, drawn from `rng` (the list is fixed: the generator is seeded with a constant)"""
    kind = kinds[int(rng.integers(0, len(kinds)))]
    kw = dict(kind=kind, fastq=bool(rng.integers(0, 2)))
    if kind == E.NS_KIND_ALIGNED:
        kw.update(chimeric=bool(rng.integers(0, 2)), emit_errlog=bool(rng.integers(0, 2)), kmer_bias=int(rng.choice([0, 0, 4, 5, 17])))
    elif kind == E.NS_KIND_PERFECT:
        kw.update(kmer_bias=int(rng.choice([0, 5])))
    return kw


def _label(i, mode, kw):
    short = {k: v for k, v in kw.items() if k not in ("seed", "max_len") and v not in (False, 0)}
    return "call %d (%s): %s" % (i, mode, short)


def _cs(a):
    a = np.ascontiguousarray(a).view(np.uint8).ravel()
    n8 = len(a) // 8 * 8
    w = a[:n8].view(np.uint64)
    return (int(np.bitwise_xor.reduce(w)) if n8 else 0, int(w.sum(dtype=np.uint64)) if n8 else 0, int(a[n8:].sum()), len(a))


def _digest(eng, b, p):
    r = b.reads()
    out = [_cs(b.records()), _cs(r), int(b.info.n_reads), int(b.info.events_used), int(b.info.total_bases)]
    if p.emit_errlog:
        out.append(_cs(b.errlog()))
    if p.meta and p.kind != E.NS_KIND_UNALIGNED:
        out.append(eng.species_bases().tobytes())
    if p.trx:
        out.append(_cs(b.polya()))
    return out


def _sample_reads(b, p, oracle_one, label, k=64):
    """k seeded reads of a big batch against the oracle, one read per oracle call (read index -> the same bytes)"""
    rng = np.random.default_rng(int(p.first_read) % (1 << 32) + int(p.n_reads))
    reads, rec = b.reads(), b.records()
    ends = np.append(reads["rec_off"].astype(np.int64)[1:], len(rec))
    for i in sorted(rng.choice(int(p.n_reads), size=min(k, int(p.n_reads)), replace=False).tolist()):
        q = E.make_params(seed=p.seed, first_read=int(p.first_read) + i, n_reads=1, kind=p.kind, fastq=p.fastq, kmer_bias=p.kmer_bias,
                          chimeric=p.chimeric, max_len=p.max_len, min_len=p.min_len, trx=p.trx, model_ir=p.model_ir)
        exp = oracle_one(q, bytes_per_read=400000, events_per_read=60000)     # (one read: the batch's shared capacity is not there)
        assert rec[int(reads["rec_off"][i]):int(ends[i])].tobytes() == exp["records"].tobytes(), "%s: sample read %d" % (label, i)
        assert int(reads["seq_len"][i]) == int(exp["reads"]["seq_len"][0]), "%s: sample read %d" % (label, i)


def _check(eng, b, p, label, oracle, fresh, one_read=True):
    """GPU batch `b` of params `p` on the long-lived engine: against the oracle (small calls) or a fresh engine (+ sample reads)"""
    if p.n_reads == 0:
        assert int(b.info.n_reads) == 0 and int(b.info.record_bytes) == 0, label
        return
    if p.n_reads <= ORACLE_MAX:
        exp = oracle(p)
        try:
            compare(b, exp, p)
        except AssertionError as err:
            raise AssertionError("%s: GPU != oracle (%s)" % (label, err)) from None
        if p.meta and p.kind != E.NS_KIND_UNALIGNED:
            assert np.array_equal(eng.species_bases(), exp["species_bases"]), label
        if p.trx:
            assert np.array_equal(b.polya(), exp["polya"]), label
        return
    got = _digest(eng, b, p)
    f = fresh()
    try:
        exp = _digest(f, f.generate(p), p)
    finally:
        f.close()
    assert got == exp, "%s: long-lived engine != fresh engine" % label
    if one_read:
        _sample_reads(b, p, oracle, label)


# ---------------------------------------------------------------------------------------------------------------------------------
# genome mode
# ---------------------------------------------------------------------------------------------------------------------------------
GENOME_SIZES = [300, 0, 4095, 1, 16385, 900, 4097, 40000, 250, 16383, 1500, 2, 600]


def _genome_calls():
    rng = np.random.default_rng(20261015)
    kinds = [E.NS_KIND_ALIGNED, E.NS_KIND_ALIGNED, E.NS_KIND_UNALIGNED, E.NS_KIND_PERFECT]
    calls = []
    for n in GENOME_SIZES:
        kw = _flags(rng, kinds)
        if kw.get("kmer_bias") and n > ORACLE_MAX:
            kw["kmer_bias"] = 5
        calls.append(dict(n_reads=n, first_read=int(rng.integers(0, 1 << 20)) + (BIG_FIRST if rng.random() < 0.3 else 0), **kw))
    # pinned: every -k value and option the issue names appears at least once (the draws above need not reach them all)
    calls[0].update(kind=E.NS_KIND_ALIGNED, kmer_bias=4, chimeric=True, fastq=True, emit_errlog=True)
    calls[2].update(kind=E.NS_KIND_ALIGNED, kmer_bias=0, chimeric=True, fastq=False, emit_errlog=True)
    calls[5].update(kind=E.NS_KIND_ALIGNED, kmer_bias=17, chimeric=False, fastq=True)
    calls[7].update(kind=E.NS_KIND_ALIGNED, kmer_bias=5, chimeric=True, fastq=True, emit_errlog=True)
    calls[9].update(kind=E.NS_KIND_UNALIGNED, kmer_bias=0, chimeric=False, emit_errlog=False)
    calls[11].update(kind=E.NS_KIND_PERFECT, kmer_bias=5, chimeric=False, emit_errlog=False)
    return calls


def _genome_failures(eng, ref, nohp_model, model):
    """calls the library refuses on the host (argument and state checks, the attempt limit): each leaves the engine usable"""
    with pytest.raises(E.EngineError):                                               # unknown kind
        p = E.make_params(seed=1, first_read=0, n_reads=10, max_len=ref.max_chrom)
        p.kind = 7
        eng.generate(p)
    with pytest.raises(E.EngineError, match="attempt limit"):                        # no read fits the length window
        eng.generate(E.make_params(seed=1, first_read=0, n_reads=10, min_len=10 ** 7, max_len=10 ** 8))
    eng.load_model(nohp_model)
    with pytest.raises(E.EngineError):                                               # -k without the homopolymer tables
        eng.generate(E.make_params(seed=1, first_read=0, n_reads=10, max_len=ref.max_chrom, kmer_bias=5))
    eng.load_model(model)


def test_genome_sequence_on_one_engine(small_model, small_ref, circ_ref):
    nohp = M.load_model(PREFIX, chimeric=True, fastq=True)
    calls = _genome_calls()
    eng = E.Engine(0)
    try:
        ref = small_ref
        eng.set_reference(ref)
        eng.load_model(small_model)
        for i, c in enumerate(calls):
            if i == 4:                                             # set_reference again, mid-sequence: the circular genome, then back
                ref = circ_ref
                eng.set_reference(ref)
            if i == 10:
                ref = small_ref
                eng.set_reference(ref)
            if i in (3, 8):                                        # a refused call between two good ones
                _genome_failures(eng, ref, nohp, small_model)
            p = E.make_params(seed=SEED + i, max_len=ref.max_chrom, **c)
            label = _label(i, "genome/%s" % ("circ" if ref is circ_ref else "linear"), c)
            r = ref

            def oracle(q, r=r, **kw):
                return O.generate(small_model, r, q, **kw)

            def fresh(r=r):
                f = E.Engine(0)
                f.set_reference(r)
                f.load_model(small_model)
                return f
            _check(eng, eng.generate(p), p, label, oracle, fresh)
    finally:
        eng.close()


def test_genome_steps_and_model_switches_on_one_engine(small_model, small_ref):
    """generate_step (the aligned call on the engine, the unaligned one on its step companion, which borrows the engine's tables) between
    plain calls, with load_model switching to the --perfect model and back; a step whose unaligned half fails on the host returns
    NS_ESTEP_UNALIGNED with a complete aligned batch, and the next step is right again"""
    perfect = M.load_model(PREFIX, perfect=True, fastq=True)
    max_len = small_ref.max_chrom

    def oracle(mdl):
        return lambda q: O.generate(mdl, small_ref, q)
    eng = E.Engine(0)
    try:
        eng.set_reference(small_ref)
        eng.load_model(small_model)
        seq = [("step", 1200, 300, dict(chimeric=True, fastq=True, emit_errlog=True)),
               ("call", 700, 0, dict(kind=E.NS_KIND_UNALIGNED, fastq=True)),
               ("model", perfect, 0, None),
               ("call", 500, 0, dict(kind=E.NS_KIND_PERFECT, fastq=True)),
               ("call", 40, 0, dict(kind=E.NS_KIND_PERFECT, first_read=BIG_FIRST)),
               ("model", small_model, 0, None),
               ("step", 400, 150, dict(kind=E.NS_KIND_PERFECT)),
               ("failstep", 800, 200, dict(kmer_bias=5, fastq=True, emit_errlog=True)),
               ("step", 2500, 600, dict(kmer_bias=4, chimeric=True, emit_errlog=True)),
               ("call", 1, 0, dict(first_read=BIG_FIRST, emit_errlog=True)),
               ("step", 300, 1, dict(first_read=BIG_FIRST + 5, fastq=True))]
        mdl = small_model
        for i, (what, n_al, n_un, kw) in enumerate(seq):
            label = "step sequence %d (%s, %s reads + %s, %s)" % (i, what, n_al if what != "model" else "-", n_un, kw)
            if what == "model":
                mdl = n_al
                eng.load_model(mdl)
                continue
            kw = dict(kw)
            first = kw.pop("first_read", 1000 * i)
            p_al = E.make_params(seed=SEED + 100 + i, first_read=first, n_reads=n_al, max_len=max_len, **kw)
            if what == "call":
                _check(eng, eng.generate(p_al), p_al, label, oracle(mdl), None)
                continue
            p_un = E.make_params(seed=SEED + 100 + i, first_read=first + n_al, n_reads=n_un, kind=E.NS_KIND_UNALIGNED, max_len=max_len,
                                 fastq=bool(kw.get("fastq")))
            if what == "failstep":
                p_un.trx = 1                                       # no transcriptome on this engine: refused on the host
                with pytest.raises(E.EngineError) as ei:
                    eng.generate_step(p_al, p_un)
                assert ei.value.code == E.NS_ESTEP_UNALIGNED, label
                assert "unaligned worker call (error %d)" % E.NS_ESTATE in str(ei.value) and "transcriptome" in str(ei.value), label
                _check(eng, ei.value.aligned_batch, p_al, label + " aligned half", oracle(mdl), None)
                continue
            b_al, b_un = eng.generate_step(p_al, p_un)
            _check(eng, b_al, p_al, label + " aligned half", oracle(mdl), None)
            _check(eng.step_engine(), b_un, p_un, label + " unaligned half", oracle(mdl), None)
        # a step whose only (unaligned) call is refused
        p_un = E.make_params(seed=SEED, first_read=0, n_reads=10, kind=E.NS_KIND_UNALIGNED, max_len=max_len, trx=True)
        with pytest.raises(E.EngineError) as ei:
            eng.generate_step(None, p_un)
        assert ei.value.code == E.NS_ESTEP_UNALIGNED and not hasattr(ei.value, "aligned_batch")
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# metagenome mode
# ---------------------------------------------------------------------------------------------------------------------------------
META_SIZES = [400, 0, 1, 4097, 1500, 16385, 300, 40000, 900, 2]


def test_metagenome_sequence_on_one_engine(small_model):
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        meta_ref = MG.read_metagenome(os.path.join(META, "genome_list.tsv"), os.path.join(META, "dna_type_list.tsv"))
    finally:
        os.chdir(cwd)
    _, samples = MG.read_abundance(os.path.join(META, "abundance.tsv"), meta_ref.species)
    perfect = M.load_model(PREFIX, perfect=True, fastq=True)
    rng = np.random.default_rng(20261016)
    kinds = [E.NS_KIND_ALIGNED, E.NS_KIND_ALIGNED, E.NS_KIND_UNALIGNED, E.NS_KIND_PERFECT]
    calls = []
    for n in META_SIZES:
        kw = _flags(rng, kinds)
        if kw["kind"] == E.NS_KIND_PERFECT:
            kw["kmer_bias"] = 0
        calls.append(dict(n_reads=n, first_read=int(rng.integers(0, 1 << 20)) + (BIG_FIRST if rng.random() < 0.3 else 0), **kw))
    calls[0].update(kind=E.NS_KIND_ALIGNED, chimeric=True, fastq=True, emit_errlog=True, kmer_bias=5)
    calls[3].update(kind=E.NS_KIND_ALIGNED, chimeric=True, fastq=True, emit_errlog=True, kmer_bias=0)
    calls[6].update(kind=E.NS_KIND_PERFECT, chimeric=False, kmer_bias=0)
    calls[7].update(kind=E.NS_KIND_ALIGNED, chimeric=False, fastq=False, emit_errlog=True, kmer_bias=0)
    calls[8].update(kind=E.NS_KIND_ALIGNED, chimeric=True, fastq=False, kmer_bias=4)
    eng = E.Engine(0)
    try:
        for i, c in enumerate(calls):
            abun = samples[0] if i < 5 else samples[1]            # a new abundance table (the next sample) mid-sequence
            infl = {sp: MG.inflate_abun(abun, sp, small_model.abun_inflation) for sp in abun}
            if i == 0:
                eng.set_metagenome(meta_ref, abun, infl)
            if i == 5:                                             # the next sample, as the CLI installs it between samples
                eng.set_abundance(meta_ref, abun, infl)
            if i in (2, 6):
                eng.load_model(small_model)
                with pytest.raises(E.EngineError):                 # perfect reads cannot be chimeric
                    eng.generate(E.make_params(seed=1, first_read=0, n_reads=10, max_len=9000, meta=True, kind=E.NS_KIND_PERFECT, chimeric=True))
                with pytest.raises(E.EngineError, match="attempt limit"):
                    eng.generate(E.make_params(seed=1, first_read=0, n_reads=10, min_len=10 ** 7, max_len=10 ** 8, meta=True))
            mdl = perfect if c["kind"] == E.NS_KIND_PERFECT else small_model
            eng.load_model(mdl)
            p = E.make_params(seed=SEED + i, max_len=meta_ref.max_chrom, meta=True, **c)
            label = _label(i, "metagenome", c)

            def oracle(q, mdl=mdl, abun=abun, infl=infl, **kw):
                return O.generate_meta(mdl, meta_ref, abun, infl if q.chimeric else None, q, **kw)

            def fresh(mdl=mdl, abun=abun, infl=infl):
                f = E.Engine(0)
                f.set_metagenome(meta_ref, abun, infl)
                f.load_model(mdl)
                return f
            _check(eng, eng.generate(p), p, label, oracle, fresh, one_read=False)
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# transcriptome mode, without and then with intron retention
# ---------------------------------------------------------------------------------------------------------------------------------
TRX_SIZES = [500, 0, 4097, 1, 4095, 16385, 300, 40000, 16383, 2500]


def test_transcriptome_sequence_on_one_engine():
    trx_ref = T.read_transcriptome(os.path.join(TRX, "transcripts.fa"), os.path.join(TRX, "expression.tsv"), os.path.join(TRX, "polya.txt"), "guppy")
    ir = IR.load(PREFIX, os.path.join(TRX, "genome.fa"), trx_ref.ref)
    tr_ir = T.restrict_expression(trx_ref, ir.eligible)
    models = {k: M.load_model(PREFIX, transcriptome=True, perfect=k == E.NS_KIND_PERFECT, fastq=True, homopolymer=k != E.NS_KIND_PERFECT)
              for k in (E.NS_KIND_ALIGNED, E.NS_KIND_PERFECT)}
    rng = np.random.default_rng(20261017)
    kinds = [E.NS_KIND_ALIGNED, E.NS_KIND_ALIGNED, E.NS_KIND_UNALIGNED, E.NS_KIND_PERFECT]
    calls = []
    for n in TRX_SIZES:
        kw = _flags(rng, kinds)
        kw.pop("chimeric", None)
        if kw["kind"] == E.NS_KIND_UNALIGNED:
            kw.update(min_len=50, max_len=5000)
        calls.append(dict(n_reads=n, first_read=int(rng.integers(0, 1 << 20)) + (BIG_FIRST if rng.random() < 0.3 else 0), **kw))
    calls[0].update(kind=E.NS_KIND_ALIGNED, kmer_bias=5, emit_errlog=True)
    calls[4].update(kind=E.NS_KIND_ALIGNED, kmer_bias=0, emit_errlog=True)
    calls[7].update(kind=E.NS_KIND_ALIGNED, kmer_bias=0, fastq=True)
    eng = E.Engine(0)
    try:
        eng.set_transcriptome(trx_ref)
        cur_ir = None
        for i, c in enumerate(calls):
            if i == 4:                                             # intron retention on, mid-sequence
                eng.set_transcriptome(tr_ir)
                eng.set_intron_retention(ir)
                cur_ir = ir
            tr = tr_ir if cur_ir is not None else trx_ref
            mdl = models[E.NS_KIND_PERFECT if c["kind"] == E.NS_KIND_PERFECT else E.NS_KIND_ALIGNED]
            eng.load_model(mdl)
            if i in (2, 6):
                with pytest.raises(E.EngineError):                 # transcriptome batches are never chimeric
                    eng.generate(E.make_params(seed=1, first_read=0, n_reads=10, max_len=9000, trx=True, chimeric=True))
                with pytest.raises(E.EngineError):                 # intron retention is a transcriptome option
                    eng.generate(E.make_params(seed=1, first_read=0, n_reads=10, max_len=9000, model_ir=True))
            kw = dict(dict(seed=SEED + i, max_len=10 ** 9, trx=True, model_ir=cur_ir is not None), **c)
            p = E.make_params(**kw)
            label = _label(i, "transcriptome%s" % (" + IR" if cur_ir is not None else ""), c)

            def oracle(q, mdl=mdl, tr=tr, ir_=cur_ir, **kw):
                return O.generate_trx(mdl, tr, q, ir=ir_ if q.model_ir else None, **kw)

            def fresh(mdl=mdl, tr=tr, ir_=cur_ir):
                f = E.Engine(0)
                f.set_transcriptome(tr)
                if ir_ is not None:
                    f.set_intron_retention(ir_)
                f.load_model(mdl)
                return f
            _check(eng, eng.generate(p), p, label, oracle, fresh)
    finally:
        eng.close()
