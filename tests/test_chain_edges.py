"""Event chains on tables whose EDGES LIE ON THE CHAIN'S OWN DRAWS.

The draws of a chain do not depend on its state: iteration `it` of piece `seg`, attempt `a`, of read `r` draws
philox(seed; it, 0, r, c3(stream, seg, a)) (philox_at of oracle/ns_oracle.c).  So instead of waiting for a 32-bit draw to land on a table
edge — once in 2^32 draws per edge — edges_on_draws() moves the edges onto the draws: every match-length column and the first-match
column get their ECDF edges on u32_to_p(w) (the draw w is the LAST of its segment) or u32_to_p(w - 1) (w is the FIRST of the next) of the
match draws, with value widths that cycle through unit, 2 .. 15, 16 and 40 (unit-wide, narrow and wide segments of ns_pack.h); the
run-length CDFs get their entries on the run-length draws in the same two placements; the mixture weights sit on a mixture draw or next to
one; the transition row of the start state has a and a + b on a draw each.  Variants: a last edge below 1 (on a draw: the clamp of
a draw above the last edge, from both sides), with and without an edge below 2^-33.

This file runs such models through the thread-per-read chains compiled for the host (tests/chain_host.hip: all five variants, staged and
unstaged, the default build and -DNS_PACK_TAIL_BITS=3) against nso_error_list / nso_unaligned_error_list, event by event;
tests/test_gpu_chain_edges.py runs them through the engine.  tests/test_lookup_probe.py covers the look-ups that can be called one draw at
a time; the straight-line block of chain_error_list and the wave-per-read lists are reached only as whole chains, hence this construction.

A test of this kind proves nothing if the chains never reach the prepared iterations, so every test counts its hits — from the oracle's
event counts, the Philox draws and the constructed tables alone, never from the code under test — and asserts at least one used draw in
every class (count_hits).

Behind them: hand chains at the bounds of the event record (a cumulative shift of exactly 2^17, a run of exactly 4 095 bases), reads whose
type draw equals one of the constant rate thresholds of the unaligned list, and the packer as a stand-alone program under sanitizers."""
import copy
import ctypes as C
import os

import numpy as np
import pytest

from nanosim_amd import model as M
from tests import oracle_lib as O
from tests.test_chain_host import ALL, HIPCC, UNALIGNED, VARIANT_FP64, _build, host_list, oracle_list, same
from tests.test_lookup_probe import GV_NARROW, GV_UNIT, Packed, build_probe, thr_gt, thr_lt, u32_to_p

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ST_EVENT, ST_UEVENT = 7, 8
NS_MIS, NS_INS, NS_DEL = 0, 1, 2
# unit, 2 .. 15 (narrow), 16 and 40 (wide: the fp64 formula); unit four times per cycle (most segments of a trained model are unit-wide,
# and a rare class needs a larger batch to be hit)
WIDTHS = (1,) + tuple(range(2, 9)) + (1,) + tuple(range(9, 16)) + (1, 16, 1, 40)
KINDS = ("unit", "narrow", "wide")
PLACES = ("last", "first")                                   # the draw is the last of its segment | the first of the next


def philox(seed, read, stream, seg, attempt, idx):
    """the four words of philox_at(d, stream, seg, attempt, idx, 0)"""
    out = (C.c_uint32 * 4)()
    c3 = ((read >> 32) & 0xff) << 24 | (stream & 0x3f) << 18 | (seg & 0xff) << 10 | (attempt & 0x3ff)
    O.lib().nso_philox(seed & 0xffffffff, (seed >> 32) & 0xffffffff, idx, 0, read & 0xffffffff, c3, out)
    return [int(x) for x in out]


def _edges(draws, widths_from=0, tiny=False):
    """(hi, vhi, {draw: (place, kind)}) of a column with one edge per draw: placements alternate, widths cycle"""
    hi, wid, on_grid, of = [], [], [], {}
    if tiny:
        hi.append(2.0 ** -34); wid.append(1); on_grid.append(False)          # threshold 0: a segment no draw reaches
    last = hi[-1] if hi else 0.0
    k = widths_from
    for j, w in enumerate(sorted(set(int(x) for x in draws))):
        place = PLACES[(j + j // len(WIDTHS)) % 2]                            # (against the widths: the other way round in the next cycle)
        u = w if place == "last" else w - 1
        if u < 0:
            continue
        width = WIDTHS[k % len(WIDTHS)]
        # the straight-line block answers from the segment word in hand: a compare that stops one segment early shows only where that
        # segment is UNIT (a narrow segment's step list gives its vhi behind its last draw, which IS the next segment's first value), so
        # every other draw that opens a segment follows a unit-wide one
        forced = place == "first" and (j // 2) % 2 == 0
        if forced:
            width = 1
        e = float(u32_to_p(u))
        # a unit-wide segment that ends exactly on a draw's probability gives vhi at that draw: ns_pack.h makes it NARROW with one step.
        # One with an even draw ends a quarter of a draw above it (the same threshold) and is UNIT — not one ulp above: behind a value edge of
        # a few thousand the formula's `+ vlo` rounds a fraction of 1 - 10^-14 up to the next whole number
        exact = width == 1 and w % 2 == 1 and not forced                      # (by the draw's own last bit: no pattern against the placements)
        if width == 1 and not exact:
            e = (u + 0.75) * 2.0 ** -32
        if e <= last:
            continue                                                          # (two draws next to each other)
        hi.append(e); wid.append(width); on_grid.append(exact or width > 1)
        of[w] = (place, len(hi) - 1)
        last = e
        k += 0 if forced else 1
    kind = ["unit" if w == 1 and not g else "narrow" if w <= 15 else "wide" for w, g in zip(wid, on_grid)]
    # the segment a draw lies in: its own (last) or the next one (first)
    cls = {}
    for w, (place, s) in of.items():
        t = s if place == "last" else s + 1
        if t < len(kind):
            cls[w] = (place, kind[t])
    return np.array(hi), np.cumsum(wid).astype(np.float64), cls, kind


class Edged:
    """the model, the draws it was built on and the class of every prepared draw"""


def edges_on_draws(mdl, seed, reads, segs, attempt, K, last_edge="one", tiny=False, n_run=300, K_match=None, aligned_segs=None):
    """a deep copy of `mdl` with its chain tables on the draws of iterations 1 .. K of stream ST_EVENT and 0 .. K of ST_UEVENT of every
    (read, seg); last_edge: "one" (1.0) or "below" (the last edge of the even columns ends on a draw that is then the last inside, that
    of the odd columns one below a draw that is then the first above); K_match: the iterations whose match draws become edges (all: K) —
    a narrow segment costs its step list, and the image is to stay the size its test wants; aligned_segs: the pieces that run the aligned
    list (all: the host build runs either list on any piece; in a batch of the engine pieces 128 .. are gaps) — the ties and the match
    edges are taken from the draws of pieces that will use them"""
    E = Edged()
    K_match = K if K_match is None else K_match
    E.seed, E.reads, E.segs, E.attempt, E.K = seed, list(reads), tuple(segs), attempt, K
    E.ev = {(r, s): np.array([philox(seed, r, ST_EVENT, s, attempt, it) for it in range(K + 1)], dtype=np.int64) for r in reads for s in segs}
    E.uv = {(r, s): np.array([philox(seed, r, ST_UEVENT, s, attempt, it) for it in range(K + 1)], dtype=np.int64) for r in reads for s in segs}
    al_keys = [k for k in E.ev if aligned_segs is None or k[1] in aligned_segs]
    un_keys = [k for k in E.uv if aligned_segs is None or k[1] not in aligned_segs]
    m = copy.deepcopy(mdl)
    nb = len(m.match_markov)
    # ---- the first-match column: the .x draws of iteration 0
    hi, vhi, E.fm_class, _ = _edges([E.ev[k][0, 0] for k in al_keys], tiny=tiny)
    if last_edge == "one":
        hi, vhi = np.append(hi, 1.0), np.append(vhi, vhi[-1] + 1)
    m.first_match = M.EcdfColumn(lo=0, hi_bin=0, hi=hi, vhi=vhi, vlo0=0.0)
    # ---- the transition row of the start state: a on an .x draw of iteration 1, a + b next to another
    x1 = np.sort(np.array([E.ev[k][1, 0] for k in al_keys]))
    xa, xb = int(x1[int(0.35 * len(x1))]), int(x1[int(0.7 * len(x1))])
    m.trans = np.array(m.trans, dtype=np.float64).copy()
    m.trans[0] = [float(u32_to_p(xa)), float(u32_to_p(xb)), float(u32_to_p(xb))]                 # (both ties ON their draws: xa is the first insertion, xb the first deletion)
    E.trans_ties = {xa, xb}

    def first_error(key):                                       # the error type of iteration 1: the oracle's trans_pick on the row above
        return int(O.lib().nso_trans_pick(np.ascontiguousarray(m.trans[0]).ctypes.data_as(C.POINTER(C.c_double)), float(u32_to_p(E.ev[key][1, 0]))))

    def u_type(key, it):                                        # S:1787 on the fixed rates of the unaligned list; 3: a match
        p = float(u32_to_p(E.uv[key][it, 0]))
        return 3 if p < 0.4 else NS_MIS if p < 0.7 else NS_INS if p < 0.85 else NS_DEL
    E.first_error, E.u_type = first_error, u_type
    # ---- mixture weights: mis on the .y draw of an aligned piece whose first error is a mismatch, ins on that of an unaligned piece whose
    # iteration 0 is an insertion, del next to (one above) the .y draw of an aligned piece whose first error is a deletion
    m.mix_w = np.array(m.mix_w, dtype=np.float64).copy()
    E.mix_ties = []                                             # (unaligned?, key, iteration, type)
    for ty, ua, beside in ((NS_MIS, False, 0), (NS_INS, True, 0), (NS_DEL, False, 1)):
        keys = [k for k in (un_keys if ua else al_keys) if (u_type(k, 0) if ua else first_error(k)) == ty]
        assert keys, "no piece draws type %d first" % ty
        k = keys[len(keys) // 2]
        y = int(E.uv[k][0, 1] if ua else E.ev[k][1, 1])
        m.mix_w[ty] = float(u32_to_p(y + beside))
        E.mix_ties.append((ua, k, 0 if ua else 1, ty))
    # ---- run-length tables: all six on the .z draws, earliest iterations first, n_run entries at most
    zu = [int(E.uv[k][it, 2]) for it in range(K + 1) for k in un_keys]
    ze = [int(E.ev[k][it, 2]) for it in range(1, K + 1) for k in al_keys]
    zs = sorted(set(zu[:n_run // 2] + ze[:n_run - n_run // 2]))                    # half from either list
    cdf, E.run_class, prev = [], {}, 0.0
    for j, w in enumerate(zs):
        place = PLACES[j % 2]
        e = float(u32_to_p(w if place == "last" else w - 1)) if (place == "last" or w > 0) else -1.0
        if e <= prev:
            continue
        cdf.append(e); E.run_class[w] = place; prev = e
    # component 1 answers one higher than component 0 (an entry no draw lies under in front), or a wrong component would go unseen
    E.run_end = {}
    if last_edge != "below":
        cdf.append(1.0)
        tabs = [cdf, [2.0 ** -34] + cdf]
    else:
        # "below": the tables are CUT, as the match columns are, so that the walk ends inside its first two reads or one step behind them:
        # the entries of the draws without a leading one bit, then two (component 0) or three (component 1) of the draws with exactly one.
        # The guide byte of that class then holds n - 2 (n - 3), and a draw of the class above the last entry walks off the table's end
        # unless `rv + 2 < n` (`rv + 1 < n` in the loop behind it) stops it — the cap at n of the oracle's table_value
        thr = thr_gt(np.array(cdf)).astype(np.int64)
        low = [e for e, t in zip(cdf, thr) if t <= 1 << 31]
        one = [(e, int(t)) for e, t in zip(cdf, thr) if 1 << 31 < t < 3 << 30]
        assert len(low) >= 2 and len(one) >= 3, "too few run-length draws with no or one leading one bit"
        tabs = [low + [e for e, _ in one[:2]], [2.0 ** -34] + low + [e for e, _ in one[:3]]]
        E.run_end = {0: one[1][1], 1: one[2][1]}                # component -> the table's last threshold
        keep = set(thr_gt(np.array(tabs[0])).astype(np.int64).tolist())
        E.run_class = {w: pl for w, pl in E.run_class.items() if (w + 1 if pl == "last" else w) in keep}
    m.mix_cdf = [[np.array(tabs[0]), np.array(tabs[1])] for _ in range(3)]
    # ---- match-length columns: the .w draws of iterations 1 .. K_match.  Which column an iteration asks depends on the chain's state —
    # except at iteration 1, where it is the bin of the first match (S:1891-1893), which the oracle's look-up gives on the column built
    # above.  So the draw of iteration 1 becomes an edge of the column that WILL be asked, and the later draws are dealt out over the
    # columns (count_hits finds out from the oracle's events which column an iteration asked): a column keeps a few dozen edges and values
    # of a few hundred (a previous match < 256 takes the straight-line path of chain_error_list).  Column b's values lie b higher than
    # its edges say.
    def first_match(key):
        fm = m.first_match
        v = int(O.lib().nso_ecdf_lookup(fm.hi.ctypes.data_as(C.POINTER(C.c_double)), fm.vhi.ctypes.data_as(C.POINTER(C.c_double)), len(fm.hi),
                                        0.0, float(u32_to_p(E.ev[key][0, 0]))))
        return max(v, 2)

    def first_col(key):
        v = first_match(key)
        for b, c in enumerate(m.match_markov):
            if c.lo <= v < c.hi_bin:
                return b
        return nb - 1
    bins = [(c.lo, c.hi_bin) for c in m.match_markov]
    E.first_match, E.first_col = first_match, first_col
    dealt = [[] for _ in range(nb)]
    for key in al_keys:
        d = E.ev[key]
        dealt[first_col(key)].append(int(d[1, 3]))
        for it in range(2, K_match + 1):
            dealt[(key[0] + it + (key[1] >> 7)) % nb].append(int(d[it, 3]))
    E.match_class, E.col_kind, E.above, E.limit, cols = [], [], {}, [None] * nb, []
    built = [_edges(dealt[b], widths_from=b, tiny=tiny) for b in range(nb)]
    cut = {}
    if last_edge == "below":
        for par, place in ((0, "last"), (1, "first")):
            cand = sorted(int(E.ev[k][1, 3]) for k in al_keys if first_col(k) % 2 == par and int(E.ev[k][1, 3]) in built[first_col(k)][2])
            assert cand, "no piece starts in a column of parity %d" % par
            w = cand[int(0.8 * (len(cand) - 1))]
            cut[par] = (w, float(u32_to_p(w if place == "last" else w - 1)))
            E.above[w] = (place, par)
    for b, (lo, hi_bin) in enumerate(bins):
        hi, vhi, cls, _ = built[b]
        if last_edge == "below":
            keep = hi < cut[b % 2][1]
            E.limit[b] = int(thr_gt(hi[keep][-1])) if keep.any() else 0      # (the classes hold for the draws below the column's new last segment)
            hi, vhi = np.append(hi[keep], cut[b % 2][1]), np.append(vhi[keep], (vhi[keep][-1] if keep.any() else 0) + 1)
        else:
            hi, vhi = np.append(hi, 1.0), np.append(vhi, vhi[-1] + 1)
        E.match_class.append(cls)
        E.col_kind.append(built[b][3])
        cols.append(M.EcdfColumn(lo=lo, hi_bin=hi_bin, hi=hi.copy(), vhi=vhi + float(b), vlo0=float(b)))
    m.match_markov = cols
    E.model = m
    return E


GUIDE_OCTAVES = 8                                               # NS_GUIDE_OCTAVES of ns_device.h


def guide_cell_start(cell):
    l, mm = cell >> 5, cell & 31
    last = 1 if l == GUIDE_OCTAVES - 1 else 0
    return ((0xffffffff00000000 >> l) & 0xffffffff) | mm << (26 + last - l)


CELL_START = np.array([guide_cell_start(c) for c in range(32 * GUIDE_OCTAVES)], dtype=np.int64)


def guide_entry(hi, w):
    """what ns_pack.h's guide holds for the cell of draw w: the segments that end below the cell's smallest draw"""
    cell = int(np.searchsorted(CELL_START, w, side="right")) - 1
    return int(np.searchsorted(hi, float(CELL_START[cell]) * 2.0 ** -32, side="left"))


def count_hits(E, pieces):
    """pieces: (read, seg, unaligned?, m_ref, events) of the ORACLE's lists at the attempt the tables were built for.  A prepared draw of
    iteration `it` counts as used when the piece certainly ran that iteration.  An unaligned list stores at most three events per
    iteration, so n_ev >= 3 it + 1 does, and its iteration 0 runs whenever m_ref > 0.  An aligned list stores one event per iteration (a
    dict-key collision takes one back), and the events tell which column every iteration asked: the match behind event k is
    pos[k + 1] - pos[k] - (the bases event k consumed), its bin is the column of iteration k + 1.  Every iteration counted is first
    checked with the ORACLE's look-up — the match it gives for that column and draw must be the one the events show — so a piece whose
    events no longer line up with its iterations (a collision) stops counting there; the last iteration of a piece has no event behind
    it to be checked against and is not counted, except iteration 1, whose column follows from the first match.
    ("run_end", component): see edges_on_draws, the cut run-length tables.
    ("line", "k0" | "k1"): the previous match is below 256, the draw EQUALS the threshold of the guide's segment | of the one behind it —
    the two compares of chain_error_list's straight-line block — and that segment is unit-wide (behind a narrow one the block's answer
    would be right by accident).  -> {list: {class: hits}}"""
    Lo = O.lib()
    al = {("match", p, k): 0 for p in PLACES for k in KINDS}
    al.update({("first_match", p): 0 for p in PLACES})
    al.update({("run", p): 0 for p in PLACES}); al.update({"mix": 0, "trans": 0, ("line", "k0"): 0, ("line", "k1"): 0})
    if E.above:
        al.update({("match", p, "above"): 0 for p in PLACES})
    if E.run_end:
        al.update({("run_end", comp): 0 for comp in E.run_end})
    un = {("run", p): 0 for p in PLACES}; un["mix"] = 0
    cols = E.model.match_markov
    thr = [thr_gt(c.hi).astype(np.int64) for c in cols]

    def bin_of(v):
        for b, c in enumerate(cols):
            if c.lo <= v < c.hi_bin:
                return b
        return len(cols) - 1
    for read, seg, unaligned, m_ref, ev in pieces:
        key, n_ev = (read, seg), len(ev)
        if unaligned:
            for it in range(E.K + 1):
                if not (m_ref > 0 and (it == 0 or n_ev >= 3 * it + 1)):
                    break
                ty = E.u_type(key, it)
                z = int(E.uv[key][it, 2])
                if ty != 3 and z in E.run_class:
                    un[("run", E.run_class[z])] += 1
                un["mix"] += sum(1 for ua, k, i, t in E.mix_ties if ua and k == key and i == it and t == ty)
            continue
        x0 = int(E.ev[key][0, 0])
        if x0 in E.fm_class:                                    # (the first match is looked up whatever the length)
            al[("first_match", E.fm_class[x0][0])] += 1
        pos = ev["pos"].astype(np.int64)
        adv = np.where(M.ev_type(ev["info"]) != NS_INS, M.ev_len(ev["info"]), 0).astype(np.int64)
        prev = E.first_match(key)
        for it in range(1, min(E.K, n_ev) + 1):
            x, y, z, w = (int(v) for v in E.ev[key][it])
            col = bin_of(prev)
            c = cols[col]
            if it < n_ev:
                seen = int(pos[it] - pos[it - 1] - adv[it - 1])
                want = int(Lo.nso_ecdf_lookup(c.hi.ctypes.data_as(C.POINTER(C.c_double)), c.vhi.ctypes.data_as(C.POINTER(C.c_double)), len(c.hi),
                                              float(c.vlo0), float(u32_to_p(w))))
                if prev == 0 and want == 0:
                    want = 1                                    # S:1900-1901
                if seen != want:
                    break
            elif it > 1:
                break
            if z in E.run_class:
                al[("run", E.run_class[z])] += 1
            if E.run_end and 1 << 31 <= z < 3 << 30:
                # a draw with one leading one bit at or above the last entry of the table the iteration asks: the type is the event's,
                # the component what the oracle's compare of the mixture draw gives
                comp = 0 if float(u32_to_p(y)) < float(E.model.mix_w[int(M.ev_type(ev["info"][it - 1]))]) else 1
                if z >= E.run_end[comp]:
                    al[("run_end", comp)] += 1
            if w in E.match_class[col] and (E.limit[col] is None or w < E.limit[col]):
                place, kind = E.match_class[col][w]
                al[("match", place, kind)] += 1
                if place == "first" and prev < 256:
                    s = int(np.searchsorted(thr[col], w, side="right"))       # the draw's segment; thr(s - 1) == w
                    d = s - 1 - guide_entry(c.hi, w)
                    if d in (0, 1) and E.col_kind[col][s - 1] == "unit":
                        al[("line", "k%d" % d)] += 1
            if w in E.above and col % 2 == E.above[w][1] and w == int(thr[col][-1]) - (1 if E.above[w][0] == "last" else 0):
                al[("match", E.above[w][0], "above")] += 1
            if it == 1:
                al["trans"] += int(x in E.trans_ties)
                al["mix"] += sum(1 for ua, k, i, t in E.mix_ties if not ua and k == key and t == E.first_error(key))
            if it < n_ev:
                prev = seen
    return dict(aligned=al, unaligned=un)


def assert_hits(hits, lists=("aligned", "unaligned")):
    for name in lists:
        empty = [k for k, v in hits[name].items() if v == 0]
        assert not empty, "the %s lists used no prepared draw of %s: %s" % (name, empty, hits[name])


# ---- CPU: the host build of the thread-per-read chains ---------------------------------------------------------------------------------
SEED, FIRST_READ, N_READS, K_ITER = 20260926, 40, 64, 8
SEGS = (0, 128)
M_REFS = (50, 400, 3000)
VARIANTS = {"one": dict(last_edge="one"), "one_tiny": dict(last_edge="one", tiny=True), "below": dict(last_edge="below"),
            "below_tiny": dict(last_edge="below", tiny=True)}


@pytest.fixture(scope="module")
def builds(tmp_path_factory):
    return dict(default=_build(str(tmp_path_factory.mktemp("chain_edges_host"))),
                tail3=_build(str(tmp_path_factory.mktemp("chain_edges_host3")), extra=("-DNS_PACK_TAIL_BITS=3",)))


@pytest.fixture(scope="module")
def edged(small_model):
    return {name: edges_on_draws(small_model, SEED, range(FIRST_READ, FIRST_READ + N_READS), SEGS, 0, K_ITER, n_run=64, **kw)
            for name, kw in VARIANTS.items()}


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return build_probe(str(tmp_path_factory.mktemp("chain_edges_probe")), gpu=False)


def test_the_packed_tables_are_what_the_construction_says(edged, probe):
    """the packer's own words: the thresholds lie on the draws (thr == w + 1 where w is the last draw of its segment, thr == w where it is
    the first of the next), and the segments have the classes count_hits files their draws under"""
    for name, E in edged.items():
        P = Packed(probe, E.model)
        try:
            assert P.whole, name
            n, seen, last = 0, set(), []
            for b, col in enumerate(E.model.match_markov):
                wb = P.words(b)
                thr = (wb & np.uint64((1 << 33) - 1)).astype(np.int64)
                kinds = np.where(wb & np.uint64(GV_UNIT), "unit", np.where(wb & np.uint64(GV_NARROW), "narrow", "wide"))
                assert np.array_equal(thr, thr_gt(col.hi).astype(np.int64))
                assert (thr[0] == 0) == ("tiny" in name)
                last.append(int(thr[-1]))
                for w, (place, kind) in E.match_class[b].items():
                    if E.limit[b] is not None and w >= E.limit[b]:
                        continue
                    s = int(np.searchsorted(thr, w, side="right"))        # the draw's segment: the first with w < thr
                    assert kinds[s] == kind, (name, b, w, place, kind, kinds[s])
                    assert (thr[s] == w + 1) if place == "last" else (s > 0 and thr[s - 1] == w), (name, b, w, place)
                    assert int(P.guide(b)[int(np.searchsorted(CELL_START, w, side="right")) - 1]) == guide_entry(col.hi, w)
                    n += 1; seen.add(kind)
            assert n > 100 and seen == set(KINDS)
            assert np.array_equal(P.cell_start, CELL_START)
            if E.above:
                for w, (place, par) in E.above.items():
                    assert all(t == (w + 1 if place == "last" else w) for t in last[par::2]), (name, w, place)
            else:
                assert set(last) == {1 << 32}
            G, _ = P.run_table(0, 0)
            G = set(G.astype(np.int64).tolist())
            assert all((z + 1 if place == "last" else z) in G for z, place in E.run_class.items())
            ties = P.blob[P.ct.trans:P.ct.trans + 2].astype(np.int64).tolist()
            assert ties[0] in E.trans_ties and ties[1] in E.trans_ties and ties[0] != ties[1]
            for ua, k, it, ty in E.mix_ties:
                y = int((E.uv if ua else E.ev)[k][it, 1])
                assert int(P.blob[P.ct.mix_w + ty]) == y + (1 if ty == NS_DEL else 0) == int(thr_lt(E.model.mix_w[ty]))
        finally:
            P.close()


@pytest.mark.parametrize("build", ["default", "tail3"])
@pytest.mark.parametrize("name", list(VARIANTS))
def test_host_chains_equal_the_oracle_with_edges_on_their_draws(builds, edged, name, build):
    L, E = builds[build], edged[name]
    t = E.model.to_c()
    keep = E.model._keep
    pk = L.chost_pack(C.byref(t))
    assert pk
    try:
        assert L.chost_whole(pk) and (L.chost_tail_bits(pk) == 3) == (build == "tail3")
        pieces = []
        for m_ref in M_REFS:
            cap = 4 * ((2 * m_ref + 64) // 4)
            for r in E.reads:
                for seg in E.segs:
                    for ua in (False, True):
                        o = oracle_list(t, ua, m_ref, E.seed, r, seg, E.attempt, cap)
                        assert not o["overflow"]
                        pieces.append((r, seg, ua, m_ref, o["ev"][:o["n_ev"]]))
                        for v in ALL:
                            if (v in UNALIGNED) != ua:
                                continue
                            for staged in ((0,) if v == VARIANT_FP64 else (0, 1)):
                                same(host_list(L, pk, v, m_ref, E.seed, r, seg, E.attempt, cap, staged=staged), o, (name, build, v, staged, m_ref, r, seg))
        # a sink of exactly the piece's size: no overflow (one slot less: overflow), on both sides
        for r in E.reads[:6]:
            for ua in (False, True):
                n_ev = oracle_list(t, ua, 3000, E.seed, r, E.segs[0], E.attempt, 8192)["n_ev"]
                for cap in (n_ev, n_ev - 1):
                    o = oracle_list(t, ua, 3000, E.seed, r, E.segs[0], E.attempt, cap)
                    assert bool(o["overflow"]) == (cap < n_ev)
                    for v in ALL:
                        if (v in UNALIGNED) == ua:
                            same(host_list(L, pk, v, 3000, E.seed, r, E.segs[0], E.attempt, cap), o, (name, build, v, "cap", cap, r))
        hits = count_hits(E, pieces)
        print(name, build, hits)
        assert_hits(hits)
    finally:
        L.chost_free(pk)
        del keep


def test_the_prepared_chains_take_every_path_of_the_straight_line_block(edged, tmp_path):
    """the counters of the chain-guide host build (NS_CHAIN_COUNT, tests/chain_guide_host.hip) over the prepared pieces: narrow segments
    answered in place, calls of next_match_gv, draws three or more segments behind the guide's entry"""
    from tests.test_chain_guide import build_host
    L = build_host(str(tmp_path))
    for name, E in edged.items():
        t = E.model.to_c()
        keep = E.model._keep
        pk = L.cg_pack(C.byref(t))
        assert pk
        try:
            counts = np.zeros(4, dtype=np.uint64)
            for r in E.reads:
                for seg in E.segs:
                    L.cg_count(pk, 3000, E.seed, r, seg, E.attempt, counts.ctypes.data)
            it, fallback, narrow, k1 = (int(x) for x in counts)
            print(name, "iterations %d, next_match_gv %d, narrow in place %d, k1 %d" % (it, fallback, narrow, k1))
            assert it >= len(E.reads) * len(E.segs) and fallback > 0 and narrow > 0 and k1 > 0, name
        finally:
            L.cg_free(pk)
            del keep


# ---- hand chains at the bounds of the event record, and the constant rates of the unaligned list --------------------------------------
RATE_DRAWS = ((20260927, 1115221799, 0.4), (20260927, 811863133, 0.7), (20260927, 284623466, 0.85))
"""(seed, read, rate): iteration 0 of piece 128 of that read draws exactly ns_thr_lt(rate) in .x — the smallest draw that is NOT below the
rate (S:1787).  The rates are constants, so no table can be moved onto a draw: these were found by a search over the 2^32 reads of four seeds."""


def test_unaligned_rates_at_a_draw_equal_to_their_threshold(builds, small_model):
    t = small_model.to_c()
    for seed, read, rate in RATE_DRAWS:
        assert philox(seed, read, ST_UEVENT, 128, 0, 0)[0] == int(thr_lt(rate)) and float(u32_to_p(int(thr_lt(rate)) - 1)) < rate
    for L in builds.values():
        pk = L.chost_pack(C.byref(t))
        try:
            for seed, read, rate in RATE_DRAWS:
                for m_ref in (1, 50):
                    o = oracle_list(t, True, m_ref, seed, read, 128, 0, 256)
                    for v in UNALIGNED:
                        for staged in (0, 1):
                            same(host_list(L, pk, v, m_ref, seed, read, 128, 0, 256, staged=staged), o, ("rate", rate, v, staged, m_ref))
        finally:
            L.chost_free(pk)


def constant_model(small_model, run, n_entries=None):
    """every iteration an insertion of `run` bases followed by a match of one base: transition rows (0, 1, 1), run-length tables whose
    entries every draw lies above (the value is the table's length), one-segment columns that give 2 (first match) and 1"""
    m = copy.deepcopy(small_model)
    m.trans = np.array([[0.0, 1.0, 1.0]] * 7)
    m.mix_cdf = [[np.concatenate([np.zeros(run - 1), [1.0]]) for _ in range(2)] for _ in range(3)]
    m.first_match = M.EcdfColumn(lo=0, hi_bin=0, hi=np.array([1.0]), vhi=np.array([3.0]), vlo0=2.0)
    m.match_markov = [M.EcdfColumn(lo=c.lo, hi_bin=c.hi_bin, hi=np.array([1.0]), vhi=np.array([2.0]), vlo0=1.0) for c in m.match_markov]
    return m


def test_a_cumulative_shift_of_exactly_two_to_the_seventeen(builds, small_model):
    """the shift in front of an event must fit 18 bits with their bias: 131 071 does, 131 072 does not (ev_shift_fits).  Insertions of 2 048
    bases one base apart: the event with index 64 has 64 x 2 048 = 2^17 in front of it, and a piece of 67 bases ends with it (66: one
    event fewer, everything fits) — `range` as the oracle sets it, on every aligned variant"""
    m = constant_model(small_model, 2048)
    t = m.to_c()
    for L in builds.values():
        pk = L.chost_pack(C.byref(t))
        try:
            assert L.chost_whole(pk)
            for m_ref, n_ev, rng in ((66, 64, False), (67, 65, True)):
                o = oracle_list(t, False, m_ref, 7, 3, 0, 0, 256)
                ev = o["ev"][:o["n_ev"]]
                assert o["n_ev"] == n_ev and bool(o["range"]) == rng and (M.ev_len(ev["info"]) == 2048).all() and (M.ev_type(ev["info"]) == NS_INS).all()
                assert int(M.ev_shift(ev["info"][-1:])[0]) == 2048 * (n_ev - 1) if not rng else True
                for v in ALL:
                    if v in UNALIGNED:
                        continue
                    for staged in ((0,) if v == VARIANT_FP64 else (0, 1)):
                        same(host_list(L, pk, v, m_ref, 7, 3, 0, 0, 256, staged=staged), o, ("shift", v, staged, m_ref))
        finally:
            L.chost_free(pk)


def test_a_run_of_exactly_the_longest_length_an_event_holds(builds, small_model):
    """NS_EV_LEN_MAX = 4 095 bases fit the event record (`range` stays clear), and a table of 4 095 entries gives exactly that for a draw
    above its last entry; 4 096 entries: one more, `range` is set.  Both as the oracle has them, on every aligned variant"""
    for run, rng in ((4095, False), (4096, True)):
        m = constant_model(small_model, run)
        t = m.to_c()
        for L in builds.values():
            pk = L.chost_pack(C.byref(t))
            try:
                for v in ALL:
                    ua = v in UNALIGNED
                    # (five bases: three insertions, far from the bound of the shift; an unaligned list merges insertions that follow
                    # each other, so its flag is whatever the oracle says)
                    o = oracle_list(t, ua, 5, 11, 5, 128 if ua else 0, 0, 256)
                    assert o["n_ev"] > 0
                    if not ua:
                        assert o["n_ev"] == 3 and bool(o["range"]) == rng and (M.ev_len(o["ev"][:3]["info"]) == 4095).all(), (run, v)
                    for staged in ((0,) if v == VARIANT_FP64 else (0, 1)):
                        same(host_list(L, pk, v, 5, 11, 5, 128 if ua else 0, 0, 256, staged=staged), o, ("run", run, v, staged))
            finally:
                L.chost_free(pk)


def test_the_packer_under_sanitizers_as_a_stand_alone_program(tmp_path):
    """ns_pack_chain_tables and ns_build_qual_lut as a stand-alone program with -fsanitize=address,undefined (tests/chain_host.hip,
    -DCHAIN_HOST_MAIN: every table in a heap buffer of exactly its size).  A loop of the packer that goes one element too far stores or
    reads behind a table and changes no answer: only this sees it"""
    import subprocess
    exe = str(tmp_path / "chain_host_main")
    subprocess.check_call([HIPCC, "--cuda-host-only", "-x", "hip", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-DNS_HOST_TEST", "-DCHAIN_HOST_MAIN",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "chain_host.hip")], cwd=ROOT)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "words" in r.stdout, (r.returncode, r.stdout[-400:], r.stderr[-2000:])
