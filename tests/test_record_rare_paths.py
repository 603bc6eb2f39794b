"""The rare-input helpers of the record kernels: iupac_members as straight-line code (nanosim_amd/csrc/ns_device.h), the ambiguity codes
of a 16-byte group / of four bases resolved by set bit (marked4, resolve16, resolve4 in nanosim_amd/csrc/ns_materialise.h) — each against a
literal copy of the form it replaced (the switch, the walk over every byte of the range), on the device source compiled for the host by
tests/record_rare_paths_host.hip.  And the reach check of tests/test_gpu_record_rare_paths.py on the oracle alone: its cases (CASES
below, shared with that file) must contain the inputs they exist for, counted with the replay of tests/kernel_classes.py plus the
counting of rare_classes() here."""
import collections
import copy
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from nanosim_amd import engine as E
from nanosim_amd import model as M
from nanosim_amd import synth
from tests import kernel_classes as K
from tests import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
needs_hipcc = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not found")

SEED = 0x5EEDC0DE5
CODES = b"YRWSKMDVHBNX"
# case_convert (S:743-755): the members of every code in the reference's list order
MEMBERS = dict(Y="CT", R="AG", W="AT", S="GC", K="TG", M="CA", D="AGT", V="ACG", H="ACT", B="CGT", N="ATCG", X="ATCG")


def build_host(tmp):
    out = os.path.join(tmp, "record_rare_paths_host.so")
    cmd = [HIPCC if os.path.exists(HIPCC) else "hipcc", "--cuda-host-only", "-x", "hip", "-O2", "-std=c++17", "-ffp-contract=off", "-DNS_HOST_TEST",
           "-shared", "-fPIC", "-o", out, os.path.join(ROOT, "tests", "record_rare_paths_host.hip")]
    subprocess.check_call(cmd, cwd=ROOT, stderr=subprocess.DEVNULL)
    L = C.CDLL(out)
    L.rr_members.restype = None; L.rr_members.argtypes = [C.c_uint32, C.c_int, C.c_void_p]
    L.rr_bytes.restype = None; L.rr_bytes.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    L.rr_marked4.restype = C.c_uint32; L.rr_marked4.argtypes = [C.c_uint32]
    L.rr_resolve16.restype = None
    L.rr_resolve16.argtypes = [C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32]
    L.rr_resolve4.restype = None
    L.rr_resolve4.argtypes = [C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32]
    return L


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_host(str(tmp_path_factory.mktemp("record_rare_paths_host")))


# ---- iupac_members ---------------------------------------------------------------------------------------------------------------
@needs_hipcc
def test_members_equal_the_switch_for_every_byte_value(host):
    """all 256 byte values (and the 256 above them: the function takes a 32-bit value) against the switch it replaced and against the
    list of case_convert written out above"""
    new, old = np.zeros(2 * 512, dtype=np.uint32), np.zeros(2 * 512, dtype=np.uint32)
    host.rr_members(512, 0, new.ctypes.data)
    host.rr_members(512, 1, old.ctypes.data)
    assert np.array_equal(new, old)
    for c in range(512):
        mem = MEMBERS.get(chr(c), "") if c < 128 else ""
        assert int(new[2 * c + 1]) == len(mem), c
        assert int(new[2 * c]) == int.from_bytes(mem.encode(), "little"), c


@needs_hipcc
def test_normalise_and_resolve_of_every_byte_value(host):
    """normalise_base keeps "anything else counts as N" (n == 0 of iupac_members), resolve_base equals its switch form for every byte
    value at 64 segment positions, and every member of every code is drawn"""
    norm = O.normalise_bases(np.arange(256, dtype=np.uint8))
    seen = collections.defaultdict(set)
    for x in range(64):
        out = np.zeros(768, dtype=np.uint8)
        host.rr_bytes(SEED, 7, 3, 1, x, out.ctypes.data)
        assert np.array_equal(out[:128] & 0x7f, norm[:128])            # the device form: the oracle's byte, bit 7 on all but ACGT
        assert np.array_equal((out[:128] & 0x80) != 0, ~np.isin(norm[:128], np.frombuffer(b"ACGT", dtype=np.uint8)))
        assert np.array_equal(out[128:256], out[:128])                 # (a reference is ASCII; the device drops bit 7 of what it reads)
        assert np.array_equal(out[256:512], out[512:])
        for c in CODES:
            seen[chr(c)].add(chr(out[256 + (c | 0x80)]))
        plain = np.arange(128)
        assert np.array_equal(out[256:384], plain)                     # without bit 7: untouched
    for code, mem in MEMBERS.items():
        assert seen[code] == set(mem), code


# ---- resolve16 / resolve4 ---------------------------------------------------------------------------------------------------------
def _groups(n, rng):
    """n groups of 16 reference bytes in device form with 0 .. 16 marked bytes (every count, every code letter), ranges, positions"""
    g = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (n, 16))].copy()
    n_marked = rng.integers(0, 17, n)
    codes = np.frombuffer(CODES, dtype=np.uint8)
    for k in range(n):
        at = rng.permutation(16)[:n_marked[k]]
        g[k, at] = codes[rng.integers(0, len(codes), len(at))] | 0x80
    i0 = rng.integers(0, 17, n).astype(np.uint32)
    i1 = rng.integers(0, 17, n).astype(np.uint32)
    i0, i1 = np.minimum(i0, i1), np.maximum(i0, i1)
    i0[: n // 8] = 0; i1[: n // 8] = 16                                   # whole chunks: the common case of a chunk lane
    x0 = rng.integers(0, 1 << 20, n).astype(np.uint32)
    return g, n_marked, i0, i1, x0


@needs_hipcc
def test_marked4(host):
    rng = np.random.default_rng(3)
    for w in [0, 0xffffffff, 0x80808080, 0x7f7f7f7f, 0x80000000, 0x00000080] + [int(x) for x in rng.integers(0, 1 << 32, 2000)]:
        exp = sum(((w >> (8 * k + 7)) & 1) << k for k in range(4))
        assert host.rr_marked4(w) == exp, hex(w)


@needs_hipcc
def test_resolve16_by_set_bit_equals_the_walk(host):
    """100 000 random groups: the tile sites' call (group masked to [i0, i1), every marked byte resolved) against the walk over every
    byte of the range"""
    rng = np.random.default_rng(20260926)
    g, n_marked, i0, i1, x0 = _groups(100_000, rng)
    assert set(n_marked) == set(range(17))
    in_range = (np.arange(16)[None, :] >= i0[:, None]) & (np.arange(16)[None, :] < i1[:, None])
    assert set(np.unique(g[(g & 0x80) != 0] & 0x7f)) == set(CODES)
    new, old = g.copy(), g.copy()
    host.rr_resolve16(len(g), 0, new.ctypes.data, i0.ctypes.data, i1.ctypes.data, x0.ctypes.data, SEED, 11, 5, 2)
    host.rr_resolve16(len(g), 2, old.ctypes.data, i0.ctypes.data, i1.ctypes.data, x0.ctypes.data, SEED, 11, 5, 2)
    assert np.array_equal(new, old)
    assert not (new & 0x80).any() and not new[~in_range].any()
    assert np.array_equal(new[in_range & ((g & 0x80) == 0)], g[in_range & ((g & 0x80) == 0)])       # plain bytes pass
    marked = in_range & ((g & 0x80) != 0)
    assert marked.sum() > 100_000 and np.isin(new[marked], np.frombuffer(b"ACGT", dtype=np.uint8)).all()
    # the dense pieces' call: the group as loaded, the first i1 bytes resolved, the others untouched
    dn = g.copy()
    zero = np.zeros(len(g), dtype=np.uint32)
    host.rr_resolve16(len(g), 1, dn.ctypes.data, zero.ctypes.data, i1.ctypes.data, x0.ctypes.data, SEED, 11, 5, 2)
    ref = g.copy()
    host.rr_resolve16(len(g), 2, ref.ctypes.data, zero.ctypes.data, i1.ctypes.data, x0.ctypes.data, SEED, 11, 5, 2)
    low = np.arange(16)[None, :] < i1[:, None]
    assert np.array_equal(dn[low], ref[low]) and np.array_equal(dn[~low], g[~low])


@needs_hipcc
def test_resolve4_by_set_bit_equals_the_walk(host):
    rng = np.random.default_rng(5)
    n = 50_000
    b = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (n, 4))].copy()
    codes = np.frombuffer(CODES, dtype=np.uint8)
    mark = rng.random((n, 4)) < 0.4
    b[mark] = codes[rng.integers(0, len(codes), int(mark.sum()))] | 0x80
    cnt = rng.integers(1, 5, n).astype(np.uint32)
    x0 = rng.integers(0, 1 << 20, n).astype(np.uint32)
    new, old = b.copy().view(np.uint32).ravel(), b.copy().view(np.uint32).ravel()
    host.rr_resolve4(n, 0, new.ctypes.data, cnt.ctypes.data, x0.ctypes.data, SEED, 13, 1, 0)
    host.rr_resolve4(n, 1, old.ctypes.data, cnt.ctypes.data, x0.ctypes.data, SEED, 13, 1, 0)
    assert np.array_equal(new, old)
    nb = new.view(np.uint8).reshape(n, 4)
    kept = np.arange(4)[None, :] < cnt[:, None]
    assert not (nb[kept] & 0x80).any() and np.array_equal(nb[~kept], b[~kept])


# ---- the cases of tests/test_gpu_record_rare_paths.py and what they must contain ----------------------------------------------------
def letters_model(base):
    """the small model with substitutions and insertions of 1 .. 20 letters, uniform (both components of the mixtures)"""
    m = copy.deepcopy(base)
    cdf = np.minimum(np.arange(1, 21, dtype=np.float64) / 20.0, 1.0)
    m.mix_cdf[K.MIS] = [cdf.copy(), cdf.copy()]
    m.mix_cdf[K.INS] = [cdf.copy(), cdf.copy()]
    return m


def build_refs():
    seq = synth.synth_sequence(60000, 31, iupac_frac=0.05)
    odd = seq.copy()                                   # X, lower-case codes and letters that are no code at all ("anything else counts as N")
    rng = np.random.default_rng(17)
    at = rng.choice(len(odd), 600, replace=False)
    odd[at] = np.frombuffer(b"XXxnyrwskmdvhbZJ*-Ue", dtype=np.uint8)[rng.integers(0, 20, len(at))]
    return dict(iupac=M.make_reference(["iupac"], [seq], "linear"), odd=M.make_reference(["odd"], [odd], "linear"),
                circ=M.read_fasta(os.path.join(GOLDEN, "genome_circ.fa"), "circular"))


def build_models(d):
    small = M.load_model(os.path.join(GOLDEN, "model_small", "training"), chimeric=True, homopolymer=True, fastq=True)
    letters = letters_model(small)
    chim = copy.deepcopy(letters)
    chim.segment_mean = 2.5
    chim.nseg_cdf = M.geometric_cdf(1.0 / 2.5, 0)
    prefix = os.path.join(str(d), "dense", "training")           # (the dense model of tests/test_gpu_kernel_classes.py)
    synth.write_model(prefix, synth.SynthModelSpec(
        n_train=3000, seed=7, aligned_median=2500.0, mis=(3.0, 0.0, 0.3, 0.5), ins=(8.0, 0.9, 0.12, 0.5), dele=(6.0, 0.95, 0.15, 0.5),
        mm_means=(2.0, 2.5, 3.0, 3.0, 3.5, 3.5, 4.0, 4.0), mm_zero=(0.0, 0.3, 0.3, 0.3, 0.3, 0.3, 0.3, 0.3), fm_mean=3.0), write_pkl=False)
    return dict(letters=letters, chim=chim, dense=M.load_model(prefix, chimeric=True, homopolymer=True, fastq=True))


CHUNK_POS = ["chunk_code_at_%d" % i for i in range(16)]
LETTER_GRID = ["letters_%s_%d_at_%d" % (t, l, o) for t in ("mis", "ins") for l in range(9, 17) for o in range(4)]
SUBST = ["sub_9_16_code_under_first", "sub_9_16_code_under_last", "sub_9_16_code_next_to", "sub_above_16_code_under_first",
         "sub_above_16_code_under_15", "sub_above_16_code_under_16", "sub_above_16_code_next_to", "sub_1_8_code_next_to"]
CHUNKS = CHUNK_POS + ["chunk_2_codes", "chunk_4_codes", "event_subrun_code_first", "event_subrun_code_last"]
# (id, reference, model, parameters, classes of rare_classes() / record_classes() / dense_classes() the case must reach)
CASES = [
    ("fasta", "iupac", "letters", dict(n_reads=300),
     CHUNKS + SUBST + LETTER_GRID + ["cut_payload_code_in_both_parts", "record:letters_cut_by_tile_end", "record:payload_continued",
                                     "record:iupac_under_substitution", "record:iupac_next_to_substitution", "record:strand_forward",
                                     "record:strand_reverse"]),
    ("fastq-errlog", "odd", "letters", dict(n_reads=200, fastq=True, emit_errlog=True), CHUNKS + SUBST + ["odd_byte_under_copy", "odd_byte_under_substitution"]),
    ("kmer-bias-5", "iupac", "letters", dict(n_reads=150, kmer_bias=5, fastq=True), []),          # (the census covers the first pass without -k)
    ("chimeric", "odd", "chim", dict(n_reads=150, chimeric=True), CHUNKS + ["record:piece_gap"]),
    ("circular", "circ", "letters", dict(n_reads=150, emit_errlog=True), ["record:piece_wraps_origin", "record:letters_slow_piece_wraps"]),
    ("unaligned-dense", "odd", "dense", dict(n_reads=150, kind=E.NS_KIND_UNALIGNED),
     ["dense:iupac_under_copy", "dense:iupac_next_to_copy", "dense:iupac_under_substitution", "dense:letters_above_4"]),
]
REACH_MIN = 4


def rare_classes(batch, ref, prm):
    """What the census of tests/kernel_classes.py does not count: where the ambiguity codes lie inside the sub-runs and under the
    substitutions of an aligned batch.  Sub-runs as the tile loop cuts them (M = ns_materialise.h, section 3a / 3b of materialise_piece): the
    copied stretch behind an event is cut at the chunk borders of the piece's chunk grid; its part in the chunk the stretch starts INSIDE
    is the event's sub-run, every other part a chunk lane's.  (A first-pass tile starts on a chunk border — test_aligned_chain_never_packs_a_chunk
    — so tiles cut no sub-run.)"""
    Cn = collections.Counter()
    plain = ~K._AMB
    for c in CODES:
        plain[c] = plain[c | 0x20] = True                      # "odd": bytes that are no code and count as N
    for r, seq, p, pq, phi in K.record_pieces(batch, prm):
        os_, pl, ty, ln, epos, rp = K._events(batch, p)
        out_len = int(p["out_len"])
        span = K._Span(ref, p)
        if span.spliced or span.wraps or not span.any_amb():
            continue
        g = (-phi) & 15
        s1 = os_ + pl
        st, en, x0 = np.concatenate([[0], s1]), np.concatenate([os_, [out_len]]), np.concatenate([[0], rp])
        cl = np.maximum(en - st, 0)
        tot = int(cl.sum())
        if tot:
            stretch = np.repeat(np.arange(len(cl)), cl)
            k = np.arange(tot) - np.repeat(np.cumsum(cl) - cl, cl)
            m = np.repeat(st, cl) + k
            x = np.repeat(x0, cl) + k
            a = span.amb(x)
            chunk, at = (m + g) >> 4, (m + g) & 15
            first_chunk = (np.repeat(st, cl) + g) >> 4
            ev_run = (stretch > 0) & (chunk == first_chunk) & (((np.repeat(st, cl) + g) & 15) != 0)
            lane = a & ~ev_run
            for i in range(16):
                Cn["chunk_code_at_%d" % i] += int((lane & (at == i)).sum())
            per = collections.Counter(zip(stretch[lane].tolist(), chunk[lane].tolist()))
            Cn["chunk_2_codes"] += sum(v >= 2 for v in per.values())
            Cn["chunk_4_codes"] += sum(v >= 4 for v in per.values())
            # first / last byte of an event sub-run: the byte at st, the byte in front of min(en, next chunk border)
            run_end = np.minimum(np.repeat(en, cl), ((chunk + 1) << 4) - g)
            Cn["event_subrun_code_first"] += int((a & ev_run & (k == 0)).sum())
            Cn["event_subrun_code_last"] += int((a & ev_run & (m == run_end - 1)).sum())
            idx = (span.pos + x) % span.chrom_len
            Cn["odd_byte_under_copy"] += int((~plain[ref.bases[span.base + idx]]).sum())
        mis = ty == K.MIS
        under = lambda off, width=1: K._window_amb(span, epos + off, np.where(mis, width, 0))
        any_under = K._window_amb(span, epos, np.where(mis, pl, 0))
        behind = K._window_amb(span, epos + pl, np.where(mis, (-pl) & 3, 0))          # the bases of the last group of four beyond the letters
        m916, m17, m18 = mis & (pl >= 9) & (pl <= 16), mis & (pl > 16), mis & (pl <= 8)
        Cn["sub_9_16_code_under_first"] += int((m916 & under(0)).sum())
        Cn["sub_9_16_code_under_last"] += int((m916 & K._window_amb(span, epos + pl - 1, np.where(mis, 1, 0))).sum())
        Cn["sub_9_16_code_next_to"] += int((m916 & behind & ~any_under).sum())
        Cn["sub_above_16_code_under_first"] += int((m17 & under(0)).sum())
        Cn["sub_above_16_code_under_15"] += int((m17 & under(15)).sum())
        Cn["sub_above_16_code_under_16"] += int((m17 & under(16)).sum())
        Cn["sub_above_16_code_next_to"] += int((m17 & behind & ~any_under).sum())
        Cn["sub_1_8_code_next_to"] += int((m18 & K._window_amb(span, epos + pl, np.where(mis, 8 - pl, 0)) & ~any_under).sum())
        if mis.any():
            for j in np.flatnonzero(mis):
                xs = (span.pos + int(epos[j]) + np.arange(int(pl[j]))) % span.chrom_len
                Cn["odd_byte_under_substitution"] += int((~plain[ref.bases[span.base + xs]]).sum())
        # the 64 classes of a payload of 9 .. 16 letters: type x length x offset of its first letter in a dword of the tile
        for t in K.piece_tiles(os_, pl, ty, rp, out_len, phi, span):
            if t["queued"]:
                continue
            j = slice(t["jb"], t["jb"] + t["cnt"])
            o, l, e_ty, e_pos = os_[j], pl[j], ty[j], epos[j]
            for tn, tv in (("mis", K.MIS), ("ins", K.INS)):
                sel = (e_ty == tv) & (l >= 9) & (l <= 16)
                for ll, oo in zip(l[sel].tolist(), ((o[sel] - t["A0"]) & 3).tolist()):
                    Cn["letters_%s_%d_at_%d" % (tn, ll, oo)] += 1
            cut = (e_ty == K.MIS) & (l > 0) & (o + l > t["M1"])                       # continued by lane 63 of the next tile
            for oo, ll, xx in zip(o[cut].tolist(), l[cut].tolist(), e_pos[cut].tolist()):
                head = t["M1"] - oo
                both = span.amb(xx + np.arange(head)).any() and span.amb(xx + head + np.arange(ll - head)).any()
                Cn["cut_payload_code_in_both_parts"] += int(both)
    return dict(Cn)


_ORACLE = {}


def oracle_case(cid, rname, mname, case, models, refs):
    """(params, oracle batch) of one case, computed once for the reach check and the GPU comparison"""
    if cid not in _ORACLE:
        kw = dict(seed=SEED, first_read=0, max_len=int(refs[rname].max_chrom))
        kw.update(case)
        p = E.make_params(**kw)
        big = p.kind == E.NS_KIND_UNALIGNED
        _ORACLE[cid] = (p, O.generate(models[mname], refs[rname], p, bytes_per_read=600000 if big else 80000, events_per_read=60000 if big else 8000))
    return _ORACLE[cid]


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    return build_models(tmp_path_factory.mktemp("record_rare_paths"))


@pytest.fixture(scope="module")
def refs():
    return build_refs()


def check_reach(cid, rname, p, exp, reach, refs):
    assert len(exp["reads"]) == p.n_reads and not exp["reads"]["flags"].any()
    cen = {}
    if p.kind == E.NS_KIND_UNALIGNED:
        cen["dense"] = K.dense_classes(exp, refs[rname].ref if hasattr(refs[rname], "ref") else refs[rname], p)
    elif not p.kmer_bias:
        cen["record"] = K.record_classes(exp, refs[rname], p)
        cen[""] = rare_classes(exp, refs[rname], p)
    for entry in reach:
        which, name = entry.split(":") if ":" in entry else ("", entry)
        assert cen[which].get(name, 0) >= REACH_MIN, "case %s reaches %s %d times" % (cid, entry, cen[which].get(name, 0))


@pytest.mark.parametrize("cid,rname,mname,case,reach", CASES, ids=[c[0] for c in CASES])
def test_cases_reach_their_classes(models, refs, cid, rname, mname, case, reach):
    """on the oracle alone: every case holds the inputs it exists for, REACH_MIN times at least"""
    p, exp = oracle_case(cid, rname, mname, case, models, refs)
    check_reach(cid, rname, p, exp, reach, refs)
