"""The WAVE-PER-READ event chains at 64 lanes without a GPU: coop_error_list, coop_unaligned_error_list and
coopk_unaligned_error_list<K>, K = 1 .. 4, of nanosim_amd/csrc/ns_chain.h — the DEVICE source — compiled for the host by
tests/chain_wave_host.hip on the lock-step wavefront of tests/wave64_host.h (64 host threads, every cross-lane primitive a rendezvous,
one CoopLds shared by the lanes, a sink per lane), against the oracle's nso_error_list / nso_unaligned_error_list event by event, with the
thread-per-read lists of the same build as a second witness.  On the GPU these lists take every long read, every unaligned read and every
gap; whole random batches (tests/test_gpu_parity.py) reach the places where their text has logic of its own by chance or never.  Here:

  - the `range` rules they restate instead of calling ev_push32 (a merged insertion above 4 095 bases; the shift in front of the first,
    second and third event of one iteration on 2^17 - 1, 2^17, -2^17, -2^17 - 1, through an initial sink shift);
  - the `overflow` rules, with sinks of n, n - 1, n - 2, n - 3, 63, 64, 65 and 0 slots and a canary behind them;
  - the block and round seams, COUNTED: a plain-Python trace of the loops (the Philox draws and the oracle's single look-ups; itself held
    against the oracle's list on every case) names what every iteration does, and a test fails when a seam class was never run;
  - K = 1, 2, 3, 4 of the template (the engine runs K = 3 and the separate one-iteration list);
  - sixteen bits: a match length of 65 534, run-length tables of 65 535 and of 65 536 entries (the last is what ns_coop_ok keeps away);
  - the stand-alone program of the build under -fsanitize=address,undefined and -fsanitize=thread, and once more with a fence() that
    orders nothing, which the thread sanitizer must refuse: a race on coop_error_list's LDS tables.
The edge tests stand first: scripts/mutation_audit.py --chain-wave runs this file with -x."""
import copy
import ctypes as C
import os
import subprocess
from collections import Counter

import numpy as np
import pytest

from nanosim_amd import model as M
from tests import oracle_lib as O
from tests.test_chain_edges import NS_DEL, NS_INS, NS_MIS, ST_EVENT, ST_UEVENT, constant_model, philox
from tests.test_chain_host import HIPCC, oracle_list, same
from tests.test_lookup_probe import _oracle, thr_lt

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

V_LDS, V_FP64, V_UNALIGNED, V_UNALIGNED_G = 0, 1, 2, 3                  # thread per read (tests/chain_host.hip)
V_COOP, V_UCOOP = 5, 6                                                  # coop_error_list, coop_unaligned_error_list
V_UCOOPK = {1: 7, 2: 8, 3: 9, 4: 10}                                    # coopk_unaligned_error_list<K>
UWAVE = (V_UCOOP,) + tuple(V_UCOOPK.values())
K_OF = {V_UCOOP: 1, 7: 1, 8: 2, 9: 3, 10: 4}
NEW = (V_COOP,) + UWAVE
BIAS = 1 << 17
SRC = os.path.join(ROOT, "tests", "chain_wave_host.hip")
LINE = ["--cuda-host-only", "-x", "hip", "-std=c++17", "-ffp-contract=off", "-DNS_HOST_TEST", "-pthread"]


def build(tmp):
    out = os.path.join(tmp, "chain_wave_host.so")
    subprocess.check_call([HIPCC, *LINE, "-O2", "-shared", "-fPIC", "-o", out, SRC], cwd=ROOT, stderr=subprocess.DEVNULL)
    L = C.CDLL(out)
    L.chost_pack.restype = C.c_void_p; L.chost_pack.argtypes = [C.POINTER(M.NsModelTables)]
    L.chost_free.restype = None; L.chost_free.argtypes = [C.c_void_p]
    L.chost_whole.restype = C.c_int; L.chost_whole.argtypes = [C.c_void_p]
    L.chost_coop_ok.restype = C.c_int; L.chost_coop_ok.argtypes = [C.POINTER(M.NsModelTables)]
    L.chost_error_list.restype = C.c_int
    L.chost_error_list.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int32, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32] + [C.c_void_p] * 6
    L.chostw_error_list.restype = C.c_int
    L.chostw_error_list.argtypes = [C.c_void_p, C.c_int, C.c_int32, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int32, C.c_void_p, C.c_uint32] + [C.c_void_p] * 6
    return L


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build(str(tmp_path_factory.mktemp("chain_wave_host")))


CANARY = 0xdeadbeef


def wave_list(L, pk, variant, m_ref, seed, read, seg, attempt, cap, shift0=0):
    """variants 5 .. 10 on the wave; 2 and 3 (thread per read) with the same initial shift.  The array carries eight canary slots behind
    its capacity, and a run whose lanes disagree or whose wave stopped is refused here"""
    ev = np.zeros(cap + 8, dtype=M.EVENT_DTYPE)
    ev["pos"][cap:] = CANARY; ev["info"][cap:] = CANARY
    out = [C.c_int32(), C.c_int32(), C.c_uint32(), C.c_int32(), C.c_int(), C.c_int()]
    rc = L.chostw_error_list(pk, variant, m_ref, seed, read, seg, attempt, shift0, ev.ctypes.data, cap, *[C.addressof(o) for o in out])
    assert rc == 0, ("the wave stopped" if rc == -2 else "the lanes end with different results" if rc == -3 else rc, variant, m_ref, seed, read)
    assert (ev["pos"][cap:] == CANARY).all() and (ev["info"][cap:] == CANARY).all(), ("a store behind the capacity", variant, m_ref, cap)
    l_new, middle_ref, n_ev, shift, overflow, rng = [o.value for o in out]
    return dict(l_new=l_new, middle_ref=middle_ref, n_ev=n_ev, shift=shift, overflow=overflow, range=rng, ev=ev[:cap])


def thread_list(L, pk, variant, m_ref, seed, read, seg, attempt, cap):
    ev = np.zeros(cap, dtype=M.EVENT_DTYPE)
    out = [C.c_int32(), C.c_int32(), C.c_uint32(), C.c_int32(), C.c_int(), C.c_int()]
    assert L.chost_error_list(pk, variant, 0, m_ref, seed, read, seg, attempt, ev.ctypes.data, cap, *[C.addressof(o) for o in out]) == 0
    l_new, middle_ref, n_ev, shift, overflow, rng = [o.value for o in out]
    return dict(l_new=l_new, middle_ref=middle_ref, n_ev=n_ev, shift=shift, overflow=overflow, range=rng, ev=ev)


def same_wave(h, o, what):
    """same(), except behind a CLIPPED event of an unaligned wave-per-read list.  The oracle and the thread-per-read lists add the 4 095
    bases an event record holds to the running shift when a merged insertion is longer; the wave-per-read unaligned lists carry the
    sum of the insertions as drawn (which is the reference's own number: it has no record to clip to).  The two differ only where
    `range` is set, and k_chain drops such a list and draws the read again, so no answer depends on it: there the lists must agree
    on the lengths, the flags, every position, length and type, and on every shift up to and including the first clipped event.
    The exception holds only for a list in which the oracle has `range` set AND an INSERTION of 4 095 bases, and only when the final
    shifts differ: every other list, a `range` from a shift term among them, is compared whole"""
    n = min(o["n_ev"], len(o["ev"]))
    info = o["ev"][:n]["info"]
    clipped = np.nonzero((M.ev_len(info) == 4095) & (M.ev_type(info) == NS_INS))[0]      # (only insertions merge; one of exactly 4 095 fits, and both sides then agree)
    if not (o["range"] and len(clipped)) or (h["range"] and h["shift"] == o["shift"]):
        return same(h, o, what)
    for k in ("l_new", "middle_ref", "n_ev"):
        assert h[k] == o[k], (what, k, h[k], o[k])
    assert bool(h["overflow"]) == bool(o["overflow"]) and bool(h["range"]), what
    first = int(clipped[0]) + 1
    assert h["ev"][:first].tobytes() == o["ev"][:first].tobytes(), what
    assert np.array_equal(h["ev"][:n]["pos"], o["ev"][:n]["pos"]) and np.array_equal(h["ev"][:n]["info"] & 0x3fff, o["ev"][:n]["info"] & 0x3fff), what


class Packed:
    def __init__(self, L, mdl):
        self.L, self.mdl, self.t = L, mdl, mdl.to_c()
        self.pk = L.chost_pack(C.byref(self.t))
        assert self.pk

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.L.chost_free(self.pk)

    def check(self, variants, unaligned, m_ref, seed, read, seg=0, attempt=0, cap=None, witness=True):
        """every variant against the oracle (and the thread-per-read list of the same build, the second witness); -> the oracle's list"""
        cap = 2 * m_ref + 64 if cap is None else cap
        o = oracle_list(self.t, unaligned, m_ref, seed, read, seg, attempt, cap)
        if witness:
            same(thread_list(self.L, self.pk, V_UNALIGNED if unaligned else V_FP64, m_ref, seed, read, seg, attempt, cap), o, ("witness", m_ref, seed, read))
        for v in variants:
            (same_wave if v in UWAVE else same)(wave_list(self.L, self.pk, v, m_ref, seed, read, seg, attempt, cap), o, (v, m_ref, seed, read, seg, attempt))
        return o


# ---- the draws and the plain-Python traces ---------------------------------------------------------------------------------------------
def philox_np(seed, read, stream, seg, attempt, idx):
    """Philox4x32-10 (Salmon et al. 2011) over an array of counter indices: what ns_draw(key, stream, seg, attempt, idx, 0) gives -> [n, 4]"""
    m32 = np.uint64(0xffffffff)
    idx = np.asarray(idx, dtype=np.uint64)
    c0, c1 = idx.copy(), np.zeros_like(idx)
    c2 = np.full_like(idx, read & 0xffffffff)
    c3 = np.full_like(idx, ((read >> 32) & 0xff) << 24 | (stream & 0x3f) << 18 | (seg & 0xff) << 10 | (attempt & 0x3ff))
    k0, k1 = seed & 0xffffffff, (seed >> 32) & 0xffffffff
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & m32, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & m32
        k0, k1 = (k0 + 0x9E3779B9) & 0xffffffff, (k1 + 0xBB67AE85) & 0xffffffff
    return np.stack([c0, c1, c2, c3], axis=1).astype(np.int64)


T04, T07, T085 = (int(thr_lt(x)) for x in (0.4, 0.7, 0.85))
MATCH = 3


def pack(ln, ty, sh):
    return (ln & 0xfff) | (ty & 3) << 12 | ((sh + BIAS) << 14) & 0xffffffff


class UTrace:
    """S:1797-1829 (unaligned_error_list) iteration by iteration: the type and step of iteration `it` follow from its draw alone (the rates
    are constants; the run length is the oracle's single look-up), the position in front of it is a running sum, and it runs in a list of
    m_ref bases exactly when that position is below m_ref.  Events as DESIGN 5.3 files them, with the shift in front of each"""
    def __init__(self, t, seed, read, seg, attempt, n_it):
        w = philox_np(seed, read, ST_UEVENT, seg, attempt, np.arange(n_it))
        x = w[:, 0]
        self.ty = np.where(x < T04, MATCH, np.where(x < T07, NS_MIS, np.where(x < T085, NS_INS, NS_DEL))).astype(np.int64)
        ask = np.where(self.ty == MATCH, NS_MIS, self.ty).astype(np.int32)
        run = np.empty(n_it, dtype=np.int64)
        u_mix, u_len = np.ascontiguousarray(w[:, 1], dtype=np.uint32), np.ascontiguousarray(w[:, 2], dtype=np.uint32)
        _oracle().nso_run_length_batch(C.byref(t), ask.ctypes.data, u_mix.ctypes.data, u_len.ctypes.data, run.ctypes.data, n_it)
        self.step = np.where(self.ty == MATCH, 1, run)
        self.seed, self.read, self.seg, self.attempt, self.n_it = seed, read, seg, attempt, n_it
        self.adv = np.where(self.ty == NS_INS, 0, self.step)
        self.pos_before = np.concatenate([[0], np.cumsum(self.adv)[:-1]])
        self.L = np.zeros(n_it, dtype=np.int64)
        self.ev_from = np.zeros(n_it + 1, dtype=np.int64)                 # events of iterations < it
        self.events, self.front = [], []                                   # (pos, type, len) and the shift in front of it
        pend, shift = 0, 0
        for it in range(n_it):
            ty, st, pos = int(self.ty[it]), int(self.step[it]), int(self.pos_before[it])
            mine = []
            if ty == NS_INS:
                pend += st
            else:
                Lp, pend = pend, 0
                self.L[it] = Lp
                if ty == MATCH:
                    mine = [(pos + 1, NS_INS, Lp)] if Lp else []
                elif ty == NS_MIS:
                    mine = [(pos, NS_MIS, st)] if not Lp else [(pos, NS_MIS, 1), (pos + 1, NS_INS, Lp)] + ([(pos + 1, NS_MIS, st - 1 - Lp)] if st - 1 > Lp else [])
                else:
                    mine = [(pos, NS_DEL, st)] if not Lp else [(pos, NS_DEL, max(st - Lp, 1))] + ([(pos + 1, NS_INS, Lp - (st - 1))] if Lp > st - 1 else [])
            for e in mine:
                self.events.append(e); self.front.append(shift)
                shift += e[2] if e[1] == NS_INS else -e[2] if e[1] == NS_DEL else 0
            self.ev_from[it + 1] = len(self.events)
        self.n_events = np.diff(self.ev_from)
        self.front = np.array(self.front + [shift], dtype=np.int64)       # (+ the shift behind the last event)
        self.ins_sum = np.concatenate([[0], np.cumsum(np.where(self.ty == NS_INS, self.step, 0))])
        self.del_sum = np.concatenate([[0], np.cumsum(np.where(self.ty == NS_DEL, self.step, 0))])
        self._need = {}

    def n_run(self, m_ref):
        n = int(np.searchsorted(self.pos_before, m_ref, side="left"))
        assert 0 < n < self.n_it - 8, "the trace is too short for this length"
        return n

    def m_ref_for(self, n):
        """the shortest list that runs exactly n iterations (its last must be one that advances), or None"""
        return int(self.pos_before[n - 1]) + 1 if 0 < n < self.n_it - 8 and self.ty[n - 1] != NS_INS else None

    def result(self, m_ref, shift0=0):
        n = self.n_run(m_ref)
        ne = int(self.ev_from[n])
        end = int(self.pos_before[n - 1] + self.adv[n - 1])
        ev = np.zeros(ne, dtype=M.EVENT_DTYPE)
        for k, ((p, ty, ln), sh) in enumerate(zip(self.events[:ne], self.front[:ne])):
            ev[k] = (p, pack(ln, ty, int(sh) + shift0))
        fits = all(-BIAS <= int(sh) + shift0 < BIAS for sh in self.front[:ne]) and all(e[2] <= 4095 for e in self.events[:ne])
        return dict(l_new=m_ref + int(self.ins_sum[n] - self.del_sum[n]) + max(0, end - m_ref), middle_ref=max(m_ref, end), n_ev=ne,
                    shift=int(self.front[ne]) + shift0, overflow=False, range=not fits, ev=ev)

    def need(self, K):
        """class -> the smallest number of run iterations with which the list has met it (None: not in this trace)"""
        if K in self._need:
            return self._need[K]
        B, ty, n_it = 64 * K, self.ty, self.n_it
        ins = ty == NS_INS
        nxt = np.full(n_it + 1, n_it, dtype=np.int64)                      # the first non-insertion iteration at or behind it
        for it in range(n_it - 1, -1, -1):
            nxt[it] = nxt[it + 1] if ins[it] else it
        need = {}

        def put(c, n):
            if n < n_it - 8 and (c not in need or n < need[c]):
                need[c] = n
        for it in range(n_it - 1):
            if ins[it]:
                if it % B == B - 1 and not ins[it + 1]:
                    put("pend0", it + 2)
                if it % B == B - 1 and it + 1 <= nxt[it + 1] < it + 1 + K:
                    put("lane0_pending", int(nxt[it + 1]) + 1)
                if it % K == K - 1:
                    put("ins_last_of_lane", int(nxt[it]) + 1)
                lane = (it % B) // K
                if it % K == 0 and 1 <= lane <= 62 and ins[it:it + K].all() and not ins[it - it % B:it].all() and nxt[it] // B == it // B:
                    put("all_ins_lane", int(nxt[it]) + 1)
            elif self.L[it] > 0:
                L, st = int(self.L[it]), int(self.step[it])
                put({MATCH: "match_L", NS_MIS: "mis3" if st - 1 > L else "mis2", NS_DEL: "del_ins" if L > st - 1 else "del_gt"}[int(ty[it])], it + 1)
        self._need[K] = need
        return need

    def classes(self, K, m_ref):
        n, B = self.n_run(m_ref), 64 * K
        c = {k for k, v in self.need(K).items() if v <= n}
        c |= {"n=0"} if n % B == 0 else {"n=1"} if n % B == 1 else {"n=-1"} if n % B == B - 1 else set()
        if n % B == 0 and int(self.pos_before[n - 1] + self.adv[n - 1]) > m_ref:
            c.add("crosses_as_last_of_round")
        if n % K:
            c.add("ends_inside_lane_%d" % (n % K))
        return c


def u_classes(K):
    return {"n=0", "n=1", "n=-1", "crosses_as_last_of_round", "pend0", "lane0_pending", "ins_last_of_lane", "all_ins_lane", "match_L", "mis2", "mis3",
            "del_gt", "del_ins"} | {"ends_inside_lane_%d" % r for r in range(1, K)}


class ATrace:
    """S:1833-1916 (error_list) with the oracle's single look-ups, iteration by iteration, for a list long enough: a shorter list runs a
    prefix of the same iterations (the loop looks at nothing but the position), so one trace serves every m_ref up to its end"""
    def __init__(self, mdl, t, seed, read, seg, attempt, n_it):
        Lo = _oracle()
        w = philox_np(seed, read, ST_EVENT, seg, attempt, np.arange(n_it + 1)).astype(np.uint32)
        one = np.empty(1, dtype=np.int64)

        def ask(f, a, u):
            a, u = np.array([a], dtype=np.int32), np.array([u], dtype=np.uint32)
            f(C.byref(t), a.ctypes.data, u.ctypes.data, one.ctypes.data, 1)
            return int(one[0])
        fm = mdl.first_match
        hi, vhi = np.ascontiguousarray(fm.hi, dtype=np.float64), np.ascontiguousarray(fm.vhi, dtype=np.float64)
        u0 = np.array([w[0, 0]], dtype=np.uint32)
        Lo.nso_ecdf_lookup_batch(hi.ctypes.data, vhi.ctypes.data, len(hi), float(fm.vlo0), u0.ctypes.data, one.ctypes.data, 1)
        prev = max(int(one[0]), 2)
        pos, state, last_ins_pos = prev, 0, -1
        self.first = prev
        self.pos_before, self.ops, self.collision, self.rule, self.delta = [], [], [], [], []
        for it in range(1, n_it + 1):
            self.pos_before.append(pos)
            err = ask(Lo.nso_trans_pick_batch, state, w[it, 0])
            a, um, ul = np.array([err], dtype=np.int32), np.array([w[it, 1]], dtype=np.uint32), np.array([w[it, 2]], dtype=np.uint32)
            Lo.nso_run_length_batch(C.byref(t), a.ctypes.data, um.ctypes.data, ul.ctypes.data, one.ctypes.data, 1)
            step = int(one[0])
            epos, coll = pos, False
            if err != NS_INS:
                pos += step
            else:
                coll = last_ins_pos == pos
                last_ins_pos = pos
            self.ops.append((epos, err, step)); self.collision.append(coll)
            self.delta.append(step if err == NS_INS else -step if err == NS_DEL else 0)
            state = 1 + err
            nm = ask(Lo.nso_next_match_batch, prev, w[it, 3])
            rule = prev == 0 and nm == 0
            if rule:
                nm = 1
            self.rule.append(rule)
            prev = nm
            pos += prev
            if prev == 0:
                state += 3
            else:
                last_ins_pos = -1
        self.pos_before.append(pos)                                       # (behind the last iteration)
        self.pos_before = np.array(self.pos_before, dtype=np.int64)
        self.n_it = n_it

    def n_run(self, m_ref):
        n = int(np.searchsorted(self.pos_before[:-1], m_ref, side="left"))
        assert n < self.n_it - 2, "the trace is too short for this length"
        return n

    def result(self, m_ref):
        n = self.n_run(m_ref)
        evs, shift, last_len, rng = [], 0, 0, False
        for it in range(n):
            epos, err, step = self.ops[it]
            if self.collision[it] and evs:                                # the dict key is taken again: the earlier insertion leaves
                evs.pop(); shift -= last_len
            ln = min(step, 4095)
            rng = rng or step > 4095 or not -BIAS <= shift < BIAS
            evs.append((epos, pack(ln, err, shift)))
            if err == NS_INS:
                shift += ln; last_len = ln
            elif err == NS_DEL:
                shift -= ln
        ev = np.zeros(len(evs), dtype=M.EVENT_DTYPE)
        for k, e in enumerate(evs):
            ev[k] = e
        end = int(self.pos_before[n]) if n else m_ref
        return dict(l_new=m_ref + sum(self.delta[:n]) + max(0, end - m_ref), middle_ref=max(m_ref, end), n_ev=len(evs), shift=shift, overflow=False,
                    range=rng, ev=ev)

    def classes(self, m_ref):
        n, c = self.n_run(m_ref), set()
        for it in range(n):                                               # block-local index: the iterations are 1-based, blocks of 64
            j = it % 64
            if self.collision[it]:
                c.add("collision_at_0_of_a_later_block" if j == 0 and it > 0 else "collision_at_a_later_index" if j else "collision_at_0_of_the_first_block")
            if self.rule[it] and j in (0, 63):
                c.add("no_two_0_matches_at_%d" % j)
        if n and n % 64 in (0, 1, 63):
            c.add("block_ends_at_i=%d" % (n % 64 or 64))
        return c


A_CLASSES = {"collision_at_0_of_a_later_block", "collision_at_a_later_index", "no_two_0_matches_at_0", "no_two_0_matches_at_63", "block_ends_at_i=1",
             "block_ends_at_i=63", "block_ends_at_i=64"}


def test_the_numpy_philox_is_the_oracles():
    w = philox_np(20260927, (5 << 32) | 77, ST_UEVENT, 130, 999, np.arange(40))
    for it in (0, 1, 17, 39):
        assert [int(x) for x in w[it]] == philox(20260927, (5 << 32) | 77, ST_UEVENT, 130, 999, it)


# ---- c. `range` ------------------------------------------------------------------------------------------------------------------------
def test_hand_chains_at_the_bounds_of_the_event_record(host, small_model):
    """the hand chains of tests/test_chain_edges.py on the wave-per-read lists: insertions of 2 048 bases one base apart — event 64, the
    first of coop_error_list's second block, has exactly 2^17 in front of it, and a piece of 67 bases ends with it (66: everything fits);
    runs of 4 095 bases fit an event, 4 096 do not"""
    with Packed(host, constant_model(small_model, 2048)) as P:
        for m_ref, n_ev, rng in ((66, 64, False), (67, 65, True)):
            o = P.check((V_COOP,), False, m_ref, 7, 3, cap=256)
            assert o["n_ev"] == n_ev and bool(o["range"]) == rng
    for run, rng in ((4095, False), (4096, True)):
        with Packed(host, constant_model(small_model, run)) as P:
            o = P.check((V_COOP,), False, 5, 11, 5, cap=256)
            assert o["n_ev"] == 3 and bool(o["range"]) == rng
            o = P.check(UWAVE, True, 5, 11, 5, seg=128, cap=256)
            assert o["n_ev"] > 0


def insertion_model(small_model, run):
    """the small model with insertions of always `run` bases (a draw above every entry of a table gives the table's length)"""
    m = copy.deepcopy(small_model)
    m.mix_cdf = [list(c) for c in m.mix_cdf]
    m.mix_cdf[NS_INS] = [np.concatenate([np.zeros(run - 1), [1.0]]) for _ in range(2)]
    return m


@pytest.mark.parametrize("run,merged_fit", [(1365, 3), (2048, 1)])
def test_a_merged_insertion_at_the_longest_length_an_event_holds(host, small_model, run, merged_fit):
    """the unaligned lists merge the insertions of consecutive iterations into one event: `bad` of the wave-per-read lists.  Tables of
    1 365 entries: three merged are 4 095 and fit, four do not; 2 048: two are 4 096.  Reads picked by their traces so that the longest
    merged insertion is exactly the last that fits, or the first that does not: both outcomes, three reads each"""
    seen, m_ref = Counter(), 40
    with Packed(host, insertion_model(small_model, run)) as P:
        for read in range(3000):
            if min(seen[False], seen[True]) >= 3:
                break
            tr = UTrace(P.t, 31, read, 128, 0, 120)
            longest = int(tr.L[:tr.n_run(m_ref)].max())
            if longest not in (run * merged_fit, run * (merged_fit + 1)) or seen[longest > 4095] >= 3:
                continue
            o = P.check(UWAVE + (V_UNALIGNED_G,), True, m_ref, 31, read, seg=128, cap=256)
            assert bool(o["range"]) == (longest > 4095) and int(M.ev_len(o["ev"][:o["n_ev"]]["info"]).max()) == min(longest, 4095)
            if not o["range"]:
                same(tr.result(m_ref), o, ("trace", run, read))
            seen[bool(o["range"])] += 1
    assert seen[False] >= 3 and seen[True] >= 3, seen


def shifted(o, shift0):
    """the oracle's list behind an initial shift: the shift fields move, `range` when a shift in front of an event leaves [-2^17, 2^17)"""
    ev = o["ev"][:o["n_ev"]].copy()
    front = M.ev_shift(ev["info"]).astype(np.int64) + shift0
    ev["info"] = (ev["info"] & np.uint32(0x3fff)) | (((front + BIAS) << 14) & 0xffffffff).astype(np.uint32)
    out = dict(o, shift=o["shift"] + shift0, range=bool(o["range"]) or bool(((front < -BIAS) | (front >= BIAS)).any()), ev=ev)
    return out, front


def test_the_shift_in_front_of_every_event_of_an_iteration_at_its_bounds(host, small_model):
    """sh, sh + d0, sh + d0 + d1: the wave-per-read unaligned lists test the shift in front of the first, second and third event of one
    iteration.  An initial sink shift puts the shift in front of a CHOSEN event on 2^17 - 1, 2^17, -2^17 and -2^17 - 1; the event is
    chosen, by a search over reads, so that it alone decides — the list ends with its iteration, and it is the first event with the largest
    (smallest) shift in front of it: the first event of an iteration for both bounds, the second (behind a deletion: sh - len) for the
    lower, the third (behind a mismatch and an insertion: sh + L) for the upper.  (The second never decides the upper bound and the
    third never the lower: the first event's shift is then at least as far out.)  In a first lane, a last lane and the first lane behind
    a round border, for every K.  The derivation — the oracle's list with the initial shift added — is first held against variants 2
    and 3, thread per read, which read s.shift through ev_track_open"""
    seed, seg, hits = 20261021, 128, Counter()
    with Packed(host, small_model) as P:
        traces = {}

        def trace(read):
            if read not in traces:
                traces[read] = UTrace(P.t, seed, read, seg, 0, 300)
            return traces[read]
        for K in (1, 2, 3, 4):
            variants = tuple(v for v in UWAVE if K_OF[v] == K)
            places = {"first_lane": range(0, K), "last_lane": range(63 * K, 64 * K), "behind_the_border": range(64 * K, 65 * K)}
            for place, its in places.items():
                for ordinal, upper in ((0, True), (0, False), (1, False), (2, True)):
                    if K == 1 and place == "first_lane" and ordinal:
                        continue                                          # (iteration 0 has no insertion in front of it: one event at most)
                    found = None
                    for read in range(6000):
                        x = philox_np(seed, read, ST_UEVENT, seg, 0, np.array(list(its)))[:, 0]
                        want_del, want_mis = ordinal == 1, ordinal == 2
                        if ordinal and not ((x >= T085) if want_del else ((x >= T04) & (x < T07))).any():
                            continue                                      # (cheap: no deletion / mismatch in the place)
                        tr = trace(read)
                        for it in its:
                            if tr.n_events[it] <= ordinal or (ordinal == 1 and tr.ty[it] != NS_DEL) or tr.m_ref_for(it + 1) is None:
                                continue
                            e, hi = int(tr.ev_from[it]) + ordinal, int(tr.ev_from[it + 1])
                            f = tr.front[:hi]
                            if (f[e] == f.max() and (f[:e] < f[e]).all()) if upper else (f[e] == f.min() and (f[:e] > f[e]).all()):
                                found = (read, it, e)
                                break
                        if found:
                            break
                        if len(traces) > 64:
                            traces.clear()
                    assert found, ("no read decides", K, place, ordinal, upper)
                    read, it, e = found
                    tr = trace(read)
                    m_ref = tr.m_ref_for(it + 1)
                    o = oracle_list(P.t, True, m_ref, seed, read, seg, 0, 1024)
                    same(tr.result(m_ref), o, ("trace", found))
                    assert not o["range"] and o["n_ev"] == tr.ev_from[it + 1]
                    at = int(M.ev_shift(o["ev"]["info"][e:e + 1])[0])
                    for target in (BIAS - 1, BIAS, -BIAS, -BIAS - 1):
                        want, front = shifted(o, target - at)
                        assert front[e] == target
                        if target in ((BIAS - 1, BIAS) if upper else (-BIAS, -BIAS - 1)):
                            assert want["range"] == (target in (BIAS, -BIAS - 1))          # this event alone decides
                        same(tr.result(m_ref, target - at), want, ("trace, shifted", found, target))
                        for v in (V_UNALIGNED, V_UNALIGNED_G) + variants:
                            same(wave_list(host, P.pk, v, m_ref, seed, read, seg, 0, 1024, shift0=target - at), want, ("shift", K, place, ordinal, upper, v, target))
                    hits[(K, place, ordinal, upper)] += 1
        # behind the LAST event of a list: the shift it ends with stands in front of no event and may be 2^17 (it is `n_ev > 2`, not
        # `>= 2`, that guards the third term).  A list that ends with an iteration of two events, the second an insertion that takes
        # the shift above everything before it
        found = None
        for read in range(2000):
            tr = trace(read)
            for it in range(3, 60):
                hi = int(tr.ev_from[it + 1])
                if tr.n_events[it] == 2 and tr.m_ref_for(it + 1) is not None and tr.front[hi] > tr.front[:hi].max():
                    found = (read, it)
                    break
            if found:
                break
        assert found, "no list ends with its largest shift behind an iteration of two events"
        read, it = found
        m_ref = trace(read).m_ref_for(it + 1)
        o = oracle_list(P.t, True, m_ref, seed, read, seg, 0, 1024)
        assert not o["range"] and o["shift"] > int(M.ev_shift(o["ev"][:o["n_ev"]]["info"]).max())
        for end in (BIAS, BIAS + 1):
            want, front = shifted(o, end - o["shift"])
            assert want["shift"] == end and bool(want["range"]) == (front.max() >= BIAS)
            assert not want["range"] if end == BIAS else True
            for v in (V_UNALIGNED, V_UNALIGNED_G) + UWAVE:
                same(wave_list(host, P.pk, v, m_ref, seed, read, seg, 0, 1024, shift0=end - o["shift"]), want, ("the shift behind the last event", v, end))
    assert len(hits) == 4 * 3 * 4 - 2, hits


def test_wave_lists_at_a_type_draw_equal_to_a_rate_threshold(host, small_model):
    """RATE_DRAWS of tests/test_chain_edges.py: iteration 0 of piece 128 draws exactly ns_thr_lt(rate), the smallest draw that is NOT below
    the rate — the `draw` lambdas of the wave-per-read lists restate S:1787"""
    from tests.test_chain_edges import RATE_DRAWS
    with Packed(host, small_model) as P:
        for seed, read, rate in RATE_DRAWS:
            assert philox(seed, read, ST_UEVENT, 128, 0, 0)[0] == int(thr_lt(rate))
            for m_ref in (0, 1, 50):
                P.check(UWAVE, True, m_ref, seed, read, seg=128, cap=256)


@pytest.mark.parametrize("run,fits", [(4097, True), (4098, False)])
def test_the_rest_of_a_mismatch_run_at_the_longest_length_an_event_holds(host, small_model, run, fits):
    """ln2, the third event of an iteration: a mismatch run of `run` bases behind an insertion of one base is filed as 1 + the insertion
    + the remaining run - 2 bases: 4 095 fit, 4 096 do not.  Reads whose first two iterations are an insertion and a mismatch"""
    m = copy.deepcopy(small_model)
    m.mix_cdf = [list(c) for c in m.mix_cdf]
    m.mix_cdf[NS_MIS] = [np.concatenate([np.zeros(run - 1), [1.0]]) for _ in range(2)]
    m.mix_cdf[NS_INS] = [np.array([1.0]) for _ in range(2)]
    n = 0
    with Packed(host, m) as P:
        for read in range(400):
            x = philox_np(41, read, ST_UEVENT, 128, 0, np.arange(2))[:, 0]
            if not (T07 <= x[0] < T085 and T04 <= x[1] < T07):
                continue
            o = P.check(UWAVE + (V_UNALIGNED_G,), True, 5, 41, read, seg=128, cap=64)
            assert o["n_ev"] == 3 and bool(o["range"]) == (not fits) and [int(v) for v in M.ev_len(o["ev"][:3]["info"])] == [1, 1, 4095]
            n += 1
    assert n >= 5


def test_coop_error_list_on_columns_of_the_other_kinds(host, small_model):
    """what the zero-match model does not have: columns whose last edge lies below 1 with a unit-wide last segment (a draw above it: the
    65 536-cell guide says `every segment passed`, and only the fallback look-up may answer); value edges that are no whole numbers
    (no integer image: the fp64 loop over the columns); tables with their edges ON the list's own draws (edges_on_draws of
    tests/test_chain_edges.py: `uu >= threshold` at equality)"""
    from tests.test_chain_edges import FIRST_READ, K_ITER, M_REFS, N_READS, SEED, SEGS, edges_on_draws
    below = zero_match_model(small_model)
    below.match_markov = [M.EcdfColumn(lo=c.lo, hi_bin=c.hi_bin, hi=np.array([0.5, 0.9]), vhi=np.array([1.0, 2.0]), vlo0=0.0) for c in below.match_markov]
    frac = zero_match_model(small_model)
    frac.match_markov = [M.EcdfColumn(lo=c.lo, hi_bin=c.hi_bin, hi=np.array([0.5, 1.0]), vhi=np.array([1.0, 4.5 + b]), vlo0=0.0) for b, c in enumerate(frac.match_markov)]
    # ... and the same with 16 columns, the most CoopLds holds: a column loop that goes one too far stores into the next lane's row
    frac16 = zero_match_model(small_model)
    edges = list(range(16)) + [40]
    frac16.match_markov = [M.EcdfColumn(lo=edges[b], hi_bin=edges[b + 1], hi=np.array([0.5, 1.0]), vhi=np.array([1.0, 4.5 + b]), vlo0=0.0) for b in range(16)]
    assert coop_ok(frac16)
    for name, mdl, whole in (("below", below, 1), ("fractional", frac, 0), ("fractional, 16 columns", frac16, 0)):
        with Packed(host, mdl) as P:
            assert host.chost_whole(P.pk) == whole, name
            assert sum(P.check((V_COOP,), False, m_ref, 9, read)["n_ev"] for read in range(12) for m_ref in (70, 400)) > 1000
    # two thresholds of one column inside ONE of the 65 536 cells of coop_error_list's guide, the draw of iteration 1 ON the second:
    # the guide's segment A ends two draws below it, B on it (`uu >= threshold` of the segment behind the guide's, at equality), both unit-wide
    for read in range(3):
        w = philox(77, read, ST_EVENT, 0, 0, 1)[3]
        assert w % 65536 >= 3
        two = copy.deepcopy(small_model)
        two.match_markov = [M.EcdfColumn(lo=c.lo, hi_bin=c.hi_bin, hi=np.array([(w - 3 + 0.75) * 2.0 ** -32, (w - 1 + 0.75) * 2.0 ** -32, 1.0]),
                                         vhi=np.array([1.0, 2.0, 3.0]), vlo0=0.0) for c in two.match_markov]
        with Packed(host, two) as P:
            assert P.check((V_COOP,), False, 400, 77, read)["n_ev"] > 1
    for kw in (dict(last_edge="one"), dict(last_edge="below", tiny=True)):
        E = edges_on_draws(small_model, SEED, range(FIRST_READ, FIRST_READ + N_READS), SEGS, 0, K_ITER, n_run=64, **kw)
        with Packed(host, E.model) as P:
            for read in E.reads:
                for m_ref in M_REFS[:2]:
                    P.check((V_COOP,), False, m_ref, SEED, read, seg=0)


# ---- d. `overflow` ---------------------------------------------------------------------------------------------------------------------
def check_caps(host, P, variants, unaligned, m_ref, seed, read, seg):
    full = oracle_list(P.t, unaligned, m_ref, seed, read, seg, 0, 4096)
    n = full["n_ev"]
    assert n > 70 and not full["overflow"]
    for cap in (n, n - 1, n - 2, n - 3, 63, 64, 65, 0):
        for v in variants:
            h = wave_list(host, P.pk, v, m_ref, seed, read, seg, 0, cap)                          # (checks the canary behind `cap`)
            for k in ("l_new", "middle_ref", "n_ev", "shift"):
                assert h[k] == full[k], (v, cap, k, h[k], full[k])
            assert bool(h["overflow"]) == (cap < n) and bool(h["range"]) == bool(full["range"]), (v, cap)
            assert h["ev"][:cap].tobytes() == full["ev"][:cap].tobytes(), (v, cap)
    return n


def test_a_sink_of_exactly_too_few_slots(host, small_model):
    """slot < cap, slot + 1 < cap, slot + 2 < cap, s.n + n_blk > cap, s.n + lane < cap: sinks of n, n - 1, n - 2, n - 3, 63, 64, 65 and 0
    slots with a canary behind them — the count and every result as with a large sink, `overflow` exactly for cap < n, the first cap events
    equal, nothing stored behind the capacity.  Unaligned reads whose LAST iteration files one, two and three events"""
    seed, seg, last = 20261022, 128, Counter()
    with Packed(host, small_model) as P:
        for read in range(400):
            if len(last) == 3:
                break
            tr = UTrace(P.t, seed, read, seg, 0, 400)
            for n in range(150, 300):
                ne, m_ref = int(tr.n_events[n - 1]), tr.m_ref_for(n)
                if m_ref is None or ne == 0 or last[ne]:
                    continue
                same(tr.result(m_ref), oracle_list(P.t, True, m_ref, seed, read, seg, 0, 4096), ("trace", read, m_ref))
                check_caps(host, P, UWAVE, True, m_ref, seed, read, seg)
                last[ne] += 1
        assert set(last) == {1, 2, 3}, last
        check_caps(host, P, (V_COOP,), False, 3000, 77, 5, 0)
    with Packed(host, zero_match_model(small_model)) as P:                # (collisions: --s.n on a sink that is full already)
        check_caps(host, P, (V_COOP,), False, 400, 77, 6, 0)


# ---- b. seams, counted -----------------------------------------------------------------------------------------------------------------
def zero_match_model(small_model):
    """a hand model whose match columns give 0 for half the draws (then 1 .. 3 + column) and whose rows draw an insertion for 40 %: an
    insertion, a match of 0 and another insertion are the dict-key collision of S:1881-1882, two draws of 0 the rule of S:1900-1901"""
    m = copy.deepcopy(small_model)
    m.trans = np.array([[0.3, 0.7, 0.7]] * 7)
    m.match_markov = [M.EcdfColumn(lo=c.lo, hi_bin=c.hi_bin, hi=np.array([0.5, 1.0]), vhi=np.array([1.0, 4.0 + b]), vlo0=0.0)
                      for b, c in enumerate(m.match_markov)]
    return m


def test_unaligned_seams_counted(host, small_model):
    """every m_ref from 1 to the end of the second round of K = 4 (512 iterations) of one read on every unaligned wave-per-read list
    against the oracle, the trace against the oracle on every case; then other reads, picked by their traces, until every seam class has
    been run by every list.  (A whole block or round of nothing but insertions — NB == 0, HAS == 0 — has a probability below 0.15^64 and
    is not chased: DESIGN section 9.)"""
    seed, seg = 20261023, 128
    counts = {v: Counter() for v in UWAVE}
    with Packed(host, small_model) as P:
        def case(tr, m_ref, variants):
            o = P.check(variants, True, m_ref, seed, tr.read, seg=seg, witness=False)
            same(tr.result(m_ref), o, ("trace", tr.read, m_ref))
            for v in variants:
                counts[v].update(tr.classes(K_OF[v], m_ref))
        tr = UTrace(P.t, seed, 1, seg, 0, 700)
        last = int(tr.pos_before[2 * 256 + 2]) + 1
        for m_ref in range(1, last + 1):
            case(tr, m_ref, UWAVE)
        assert tr.n_run(last) >= 2 * 256 + 2
        for K in (1, 2, 3, 4):
            variants, B = tuple(v for v in UWAVE if K_OF[v] == K), 64 * K
            for read in range(2, 400):
                missing = u_classes(K) - set(counts[variants[0]])
                if not missing:
                    break
                tr = UTrace(P.t, seed, read, seg, 0, 700)
                cand = {v for c, v in tr.need(K).items() if c in missing} | {B - 1, B, B + 1, 2 * B - 1, 2 * B, 2 * B + 1} | set(range(B + 1, B + K))
                for n in sorted(cand):
                    m_ref = tr.m_ref_for(n)
                    if m_ref is not None and tr.classes(K, m_ref) & (u_classes(K) - set(counts[variants[0]])):
                        for mr in (m_ref - 1, m_ref, m_ref + 1):
                            case(tr, mr, variants)
    for v in UWAVE:
        empty = u_classes(K_OF[v]) - {k for k, n in counts[v].items() if n > 0}
        print(v, dict(counts[v]))
        assert not empty, (v, empty)


def test_aligned_seams_counted(host, small_model):
    """coop_error_list on the zero-match hand model: every m_ref over the first two blocks of one read, then reads picked by their traces
    until a collision at block-local index 0 with events filed (--s.n takes back an event that is in global memory already), one at a
    later index, the rule "no two 0-matches" at index 0 and 63, and blocks that end at i = 1, 63 and 64 have all been run"""
    seed, counts = 20261024, Counter()
    mdl = zero_match_model(small_model)
    with Packed(host, mdl) as P:
        def case(tr, m_ref):
            o = P.check((V_COOP,), False, m_ref, seed, tr.read, cap=1024)
            same(tr.result(m_ref), o, ("trace", tr.read, m_ref))
            counts.update(tr.classes(m_ref))
        tr = ATrace(mdl, P.t, seed, 1, 0, 0, 160); tr.read = 1
        for m_ref in range(1, int(tr.pos_before[132]) + 1):
            case(tr, m_ref)
        for read in range(2, 300):
            if not A_CLASSES - set(counts):
                break
            tr = ATrace(mdl, P.t, seed, read, 0, 0, 160); tr.read = read
            for n in (1, 63, 64, 65, 66, 127, 128, 129, 130):
                m_ref = int(tr.pos_before[n - 1]) + 1
                if tr.n_run(m_ref) == n and tr.classes(m_ref) & (A_CLASSES - set(counts)):
                    for mr in (m_ref - 1, m_ref, m_ref + 1):
                        case(tr, mr)
    print(dict(counts))
    assert not A_CLASSES - set(counts), A_CLASSES - set(counts)


# ---- e. sixteen bits -------------------------------------------------------------------------------------------------------------------
def coop_ok(mdl):
    """the gate of ns_load_model (ns_coop_ok, ns_pack.h), restated"""
    vmax = max(float(c.vhi.max()) for c in mdl.match_markov)
    return len(mdl.match_markov) <= 16 and vmax < 65535.0 and max(len(c) for ty in mdl.mix_cdf for c in ty) <= 65535


def sixteen_bin_model(small_model, nbins=16, top=65534.0):
    """nbins columns; the last bin's column gives top - 1 for half the draws and top for the other half"""
    m = copy.deepcopy(small_model)
    edges = list(range(nbins)) + [40]                                   # (top lies above every bin: the walk of S:1891-1893 ends without a hit, the last bin)
    m.match_markov = [M.EcdfColumn(lo=edges[b], hi_bin=edges[b + 1], hi=np.array([0.5, 1.0]),
                                   vhi=np.array([top, top]) if b == nbins - 1 else np.array([1.0 + b, 40.0 + b]),
                                   vlo0=top - 1 if b == nbins - 1 else float(b)) for b in range(nbins)]
    return m


def test_sixteen_bits_of_a_match_and_of_a_run_length(host, small_model):
    """coop_error_list keeps the next match of every column and the run length of every type in 16 bits.  The largest model ns_coop_ok
    admits: 16 columns, matches of 65 534; run-length tables of 65 535 entries (a draw above the last entry gives the table's length).
    One of 65 536 entries comes back from the uint16_t as a step of 0 (m_ref 40, seed 11, read 5: 38 events of length 0, l_new 40 and no
    `range`, where the oracle has 38 clipped events, l_new 2 490 408 and `range`) — so ns_coop_ok refuses such a model, and every read
    stays on the thread-per-read lists, which equal the oracle there"""
    mdl = sixteen_bin_model(small_model)
    with Packed(host, mdl) as P:
        assert coop_ok(mdl) and host.chost_coop_ok(C.byref(P.t)) == 1
        big = 0
        for read in range(6):
            o = P.check((V_COOP,), False, 3000000, 5, read, cap=4096)
            big += int((np.diff(o["ev"][:o["n_ev"]]["pos"].astype(np.int64)) >= 65533).sum())
        assert big > 20                                                   # matches of 65 533 and 65 534 were drawn
    for nbins, top, ok in ((17, 65534.0, False), (16, 65535.0, False), (16, 60000.0, True)):
        mdl = sixteen_bin_model(small_model, nbins, top)
        t = mdl.to_c()
        assert coop_ok(mdl) == ok and host.chost_coop_ok(C.byref(t)) == int(ok), (nbins, top)
    for run, ok in ((65535, True), (65536, False)):
        mdl = constant_model(small_model, run)
        with Packed(host, mdl) as P:
            assert coop_ok(mdl) == ok and host.chost_coop_ok(C.byref(P.t)) == int(ok), run
            o = P.check((V_COOP,) if ok else (), False, 40, 11, 5, cap=256)          # (the witnesses: variant 1; and variant 0 below)
            same(thread_list(host, P.pk, V_LDS, 40, 11, 5, 0, 0, 256), o, ("thread per read", run))
            assert o["n_ev"] > 10 and o["range"] and o["l_new"] == 40 + run * o["n_ev"]
            if not ok:                                                    # what the gate guards against: the list itself, asked all the same
                h = wave_list(host, P.pk, V_COOP, 40, 11, 5, 0, 0, 256)
                assert h["n_ev"] == o["n_ev"] and not h["range"] and h["l_new"] == 40 and (M.ev_len(h["ev"][:h["n_ev"]]["info"]) == 0).all()


# ---- a. sweeps -------------------------------------------------------------------------------------------------------------------------
def sweep(host, mdl, n_cases, seed, lengths, long_once):
    n_events = 0
    with Packed(host, mdl) as P:
        rng = np.random.default_rng(seed)
        for i in range(n_cases):
            m_ref = int(lengths[i % len(lengths)]) if i < 2 * len(lengths) else int(rng.integers(1, max(lengths) + 1))
            sd, rd = int(rng.integers(0, 2 ** 63)), int(rng.integers(0, 2 ** 40))
            seg, att = int(rng.choice([0, 1, 5, 128, 130])), int(rng.integers(0, 1000))
            n_events += P.check((V_COOP,), False, m_ref, sd, rd, seg=seg, attempt=att)["n_ev"]
            n_events += P.check(UWAVE, True, m_ref, sd, rd, seg=seg, attempt=att)["n_ev"]
        P.check((V_COOP,), False, long_once, seed, 9)
        P.check(UWAVE, True, long_once, seed, 9, seg=128)
        assert host.chost_whole(P.pk)
    return n_events


LENGTHS = (0, 1, 2, 3, 7, 50, 400, 3000)            # (0: an empty gap — the wave-per-read lists must leave before their first round)


def test_wave_chains_on_the_small_model(host, small_model):
    assert sweep(host, small_model, 200, 1, LENGTHS, 20000) > 60000


@pytest.mark.parametrize("name", ["dense", "big", "long"])
def test_wave_chains_on_models_that_take_the_other_look_up_paths(host, tmp_path, name):
    """the dense model (an event every ~3 bases, zero-length matches, collisions) and the trained-model shape (15 bins of 1 500-row ECDFs:
    coop_error_list's 65 536-cell guide and its ecdf_lookup_gv fallback) of tests/test_chain_host.py"""
    from nanosim_amd import synth
    bins = ((0, 1), (1, 2), (2, 3), (3, 5), (5, 7), (7, 10), (10, 14), (14, 19), (19, 25), (25, 33), (33, 45), (45, 60), (60, 90), (90, 150), (150, 1500))
    spec = dict(big=synth.SynthModelSpec(n_train=3000, seed=99, ecdf_rows=1500, mm_bins=bins, mm_means=tuple(20.0 + 2 * i for i in range(15)),
                                         mm_zero=(0.0,) + (0.02,) * 14, fm_mean=25.0),
                # (matches of hundreds of bases: the bin walk behind bin_lut, with bin edges at 256, 700, 1001, 2048)
                long=synth.SynthModelSpec(n_train=3000, seed=11, ecdf_rows=3000, fm_mean=150.0,
                                          mm_bins=((0, 40), (40, 120), (120, 256), (256, 700), (700, 1001), (1001, 2048), (2048, 3000)),
                                          mm_means=(150.0, 200.0, 260.0, 320.0, 380.0, 430.0, 480.0), mm_zero=(0.0,) + (0.01,) * 6),
                dense=synth.SynthModelSpec(n_train=3000, seed=7, aligned_median=2500.0, mis=(3.0, 0.0, 0.3, 0.5), ins=(8.0, 0.9, 0.12, 0.5),
                                           dele=(6.0, 0.95, 0.15, 0.5), mm_means=(2.0, 2.5, 3.0, 3.0, 3.5, 3.5, 4.0, 4.0),
                                           mm_zero=(0.0, 0.3, 0.3, 0.3, 0.3, 0.3, 0.3, 0.3), fm_mean=3.0))[name]
    prefix = str(tmp_path / name / "training")
    synth.write_model(prefix, spec, write_pkl=False)
    assert sweep(host, M.load_model(prefix), 40 if name == "long" else 100, 2, LENGTHS + ((9000,) if name == "long" else ()), 20000) > (3000 if name == "long" else 20000)


# ---- f. sanitizers, as stand-alone programs only ---------------------------------------------------------------------------------------
def program(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.check_call([HIPCC, *LINE, "-O1", "-g", "-DCHAIN_WAVE_MAIN", *flags, "-fno-sanitize-recover=all", "-o", exe, SRC], cwd=ROOT, stderr=subprocess.DEVNULL)
    return exe


@pytest.mark.parametrize("sanitize", ["address,undefined", "thread"])
def test_wave_program_is_clean_under_the_sanitizers(tmp_path, sanitize):
    """tests/chain_wave_host.hip with its own main (-DCHAIN_WAVE_MAIN), started as a child process: a hand model packed into heap buffers of
    exactly their size, the three lists (K = 1 .. 4) on seam, cap and shift cases against the thread-per-read lists of the same program.
    address,undefined: no lane reads behind the copy of the LDS words or stores behind a sink.  thread: no two lanes store to one event
    slot, and CoopLds is written and read only across fence() — the one collective of the host wave that orders memory (next test)"""
    r = subprocess.run([program(tmp_path, "chain_wave_" + sanitize.split(",")[0], ["-fsanitize=" + sanitize])], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "cases equal" in r.stdout, (r.returncode, r.stdout[-400:], r.stderr[-3000:])


def test_thread_sanitizer_refuses_coop_error_list_without_its_fences(tmp_path):
    """what the clean -fsanitize=thread run is worth: built with a fence() that orders nothing (-DWAVE64_FENCE_ORDERS_NOTHING), the same
    program is refused — a data race on the LDS tables of coop_error_list, which one lane fills and every lane walks"""
    r = subprocess.run([program(tmp_path, "chain_wave_thread_nofence", ["-fsanitize=thread", "-DWAVE64_FENCE_ORDERS_NOTHING"])], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "ThreadSanitizer: data race" in r.stderr and "coop_error_list" in r.stderr, (r.returncode, r.stderr[-3000:])
