"""GPU == oracle at the operating points the record kernels are not tuned for (nanosim_amd.synth.OPERATING_POINTS): a sparse-error model
(q20_like, ~100 events per 8.4 kb read), a dense one (r9_like, ~700) and an ultra-long one (ul_like, aligned median 35 kb), each on a
linear and a circular reference, and each in one batch big enough for the cooperative chain at the default coop_min / coop_shift.
Every test asserts that it reached the edge it is about; a case that does not reach it fails.

The slow-tile count is derived on the host: the record kernel closes a tile of T_OUT = 2048 output bytes early when more than 63 events
start in it and queues the rest.  A piece's events are counted per 2048-base window of its reference span (event `pos`), the output
tiles' size in bases of the read."""
import os

import numpy as np
import pytest

from nanosim_amd import engine as E
from nanosim_amd import model as M
from nanosim_amd import synth
from tests import oracle_lib as O
from tests.test_gpu_parity import compare

pytestmark = pytest.mark.gpu
T_OUT, TILE_EVENTS = 2048, 63
COOP_MIN = 16384                  # the default coop_min: a batch this size puts its longest reads on the cooperative chain


@pytest.fixture(scope="module")
def op_models(tmp_path_factory):
    out = {}
    for name in synth.OPERATING_POINTS:
        prefix = str(tmp_path_factory.mktemp(name) / "training")
        synth.write_model(prefix, synth.operating_point_spec(name), write_pkl=False)
        out[name] = M.load_model(prefix, chimeric=True, homopolymer=True, fastq=True)
    return out


@pytest.fixture(scope="module")
def ul_refs():
    """references long enough for ul_like reads: a linear genome of 2 Mb and a circular one of 500 kb (seeded)"""
    lin, circ = 2_000_000, 500_000
    a = synth.synth_sequence(lin, 20261104, hp_boost=0.005)
    b = synth.synth_sequence(circ, 20261105, hp_boost=0.005)
    return (M.Reference(["ul_linear"], a, np.array([0, lin], dtype=np.uint64), np.array([0], dtype=np.uint8)),
            M.Reference(["ul_circular"], b, np.array([0, circ], dtype=np.uint64), np.array([1], dtype=np.uint8)))


def _refs(name, small_ref, circ_ref, ul_refs):
    return ul_refs if name == "ul_like" else (small_ref, circ_ref)


def _window_counts(pieces, events):
    """events per 2048-base window of every aligned piece (full windows, and the piece's last partial one)"""
    full, tail = [], []
    for pc in pieces[(pieces["kind"] == 0) & (pieces["ref_len"] > 0)]:
        ev = events[int(pc["ev_off"]):int(pc["ev_off"]) + int(pc["n_ev"])]
        nw = (int(pc["ref_len"]) + T_OUT - 1) // T_OUT
        c = np.bincount(np.minimum(ev["pos"].astype(np.int64) // T_OUT, nw - 1), minlength=nw)
        if int(pc["ref_len"]) % T_OUT:
            tail.append(int(c[-1]))
            c = c[:-1]
        full.extend(c.tolist())
    return np.array(full, dtype=np.int64), np.array(tail, dtype=np.int64)


CASES = [dict(emit_errlog=True), dict(chimeric=True, fastq=True, emit_errlog=True), dict(kmer_bias=5, fastq=True),
         dict(kind=E.NS_KIND_UNALIGNED, fastq=True)]


@pytest.mark.parametrize("name", list(synth.OPERATING_POINTS))
def test_operating_point_equals_oracle(op_models, small_ref, circ_ref, ul_refs, name):
    """FASTA + error profile, chimeric FASTQ, -k 5 FASTQ and unaligned reads at each operating point, linear and circular reference.
    Reached: r9_like -- most full tiles past the 63-event limit (the slow-tile queue); q20_like -- no full tile past the limit, a median
    of at most 32 events per full tile, and tiles without any event (a piece's last, partial tile: full ones hold ~25 on average); ul_like -- a piece of 100 kb or more, a piece across the circular origin, and n_range_redraws == 0 as in the
    oracle (its match lengths stay within the model's 200-row ECDF, far below the 4 095-base run limit of the event record, and no
    segment's indel balance nears +-131 071, so neither side redraws: both give the same reads, which compare() checks)."""
    mdl = op_models[name]
    n = 100 if name == "ul_like" else 300
    full, tail, max_ref, across, redraws = [], [], 0, 0, 0
    for ref in _refs(name, small_ref, circ_ref, ul_refs):
        e = E.Engine(0)
        try:
            e.set_reference(ref)
            e.load_model(mdl)
            for i, case in enumerate(CASES):
                p = E.make_params(**dict(dict(seed=0x0BE7A000 + i, first_read=7, n_reads=n, max_len=ref.max_chrom), **case))
                b = e.generate(p)
                exp = O.generate(mdl, ref, p, **O.sizes_for_model(mdl, p))
                try:
                    compare(b, exp, p)
                except AssertionError as err:
                    raise AssertionError("%s, %s, %s: GPU != oracle (%s)" % (name, ref.names[0], case, err)) from None
                pc, ev = b.pieces(), b.events()
                redraws += int(b.info.n_range_redraws)
                if p.kind == E.NS_KIND_ALIGNED and not p.kmer_bias:
                    f, t = _window_counts(pc, ev)
                    full.append(f)
                    tail.append(t)
                al = pc[pc["kind"] == 0]
                max_ref = max(max_ref, int(al["ref_len"].max()) if len(al) else 0)
                if ref.circular[0]:
                    across += int(np.sum(pc["pos"].astype(np.int64) + pc["ref_len"] > ref.genome_len))
        finally:
            e.close()
    full, tail = np.concatenate(full), np.concatenate(tail)
    assert len(full) > 100, "too few full tiles to say anything"
    if name == "r9_like":
        assert np.mean(full > TILE_EVENTS) > 0.5, "r9_like: most full tiles should pass the 63-event limit (slow-tile queue)"
    if name == "q20_like":
        assert np.max(full) <= TILE_EVENTS and np.median(full) <= 32, "q20_like: tiles are not sparse"
        assert np.sum(tail == 0) > 0, "q20_like: no tile without events"
    if name == "ul_like":
        assert max_ref >= 100_000, "ul_like: no piece of 100 kb or more (longest %d)" % max_ref
        assert across > 0, "ul_like: no piece crossed the circular origin"
    assert redraws == 0


@pytest.mark.parametrize("name", list(synth.OPERATING_POINTS))
def test_operating_point_cooperative_chain(op_models, small_ref, ul_refs, name):
    """One batch of COOP_MIN reads at the default coop_min / coop_shift: its longest reads take the cooperative (wave-per-read) chain.
    256 seeded sample reads of it equal the oracle's, and the same reads in batches of 4 096 (below coop_min: the thread-per-read list
    only) give the same records byte for byte."""
    mdl = op_models[name]
    ref = ul_refs[0] if name == "ul_like" else small_ref
    e = E.Engine(0)
    try:
        e.set_reference(ref)
        e.load_model(mdl)
        p = E.make_params(seed=0x0C00B000, first_read=(1 << 32) + 3, n_reads=COOP_MIN, max_len=ref.max_chrom)
        b = e.generate(p)
        reads, rec = b.reads(), b.records()
        assert int(b.info.n_range_redraws) == 0
        ends = np.append(reads["rec_off"].astype(np.int64)[1:], len(rec))
        rng = np.random.default_rng(20261106)
        for i in sorted(rng.choice(COOP_MIN, size=256, replace=False).tolist()):
            q = E.make_params(seed=p.seed, first_read=int(p.first_read) + i, n_reads=1, max_len=ref.max_chrom)
            exp = O.generate(mdl, ref, q, **O.sizes_for_model(mdl, q))
            assert rec[int(reads["rec_off"][i]):int(ends[i])].tobytes() == exp["records"].tobytes(), "%s: read %d" % (name, i)
        # the longest reads of the batch are among the samples' equals: compare them against the oracle as well
        for i in np.argsort(reads["seq_len"])[-8:].tolist():
            q = E.make_params(seed=p.seed, first_read=int(p.first_read) + i, n_reads=1, max_len=ref.max_chrom)
            exp = O.generate(mdl, ref, q, **O.sizes_for_model(mdl, q))
            assert rec[int(reads["rec_off"][i]):int(ends[i])].tobytes() == exp["records"].tobytes(), "%s: long read %d" % (name, i)
        big = rec.tobytes()
        del rec
        totals = (int(b.info.events_used), int(b.info.total_bases), int(b.info.total_ref_bases))
        off, sums = 0, np.zeros(3, dtype=np.int64)
        for k in range(COOP_MIN // 4096):
            q = E.make_params(seed=p.seed, first_read=int(p.first_read) + 4096 * k, n_reads=4096, max_len=ref.max_chrom)
            bq = e.generate(q)
            part = bq.records().tobytes()
            assert part == big[off:off + len(part)], "%s: batch %d of 4 096 differs from the big batch" % (name, k)
            off += len(part)
            sums += (int(bq.info.events_used), int(bq.info.total_bases), int(bq.info.total_ref_bases))
        assert off == len(big)
        assert tuple(sums.tolist()) == totals, "%s: events_used / total bases of the big batch != the sum over its 4 096-read batches" % name
    finally:
        e.close()
