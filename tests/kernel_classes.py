"""The census of input classes of the three kernels that write almost every output byte: the tile loop of
k_materialise (materialise_piece, nanosim_amd/csrc/ns_materialise.h), the body of k_materialise_dense (dense_piece, same file) and
k_errlog<BUF> (nanosim_amd/csrc/nanosim_amd.hip).  A helper, not a test: numpy and the standard library only.

Which branch these kernels take is a pure function of the batch: the first output offset, length and type of every event, the piece
lengths, where the sequence line lands modulo 16 in the record image, the read-name length.  The functions below replay the CASE
SELECTION of the kernels over an oracle batch (the dict tests.oracle_lib.generate / generate_meta / generate_trx return) and count
how often every class occurs — never their data path: no byte of output is computed here, so the census cannot agree with a kernel
by sharing its mistake.  Every counter names, in a comment, the source line of the branch it drives ("M:" = ns_materialise.h,
"H:" = nanosim_amd.hip).

    record_classes(batch, ref, prm)   first record pass (MAT_REF) of an aligned / perfect batch: every piece the tile loop takes
    dense_classes(batch, ref, prm)    batches of unaligned reads (the only batches launch_materialise gives to k_materialise_dense)
    errlog_classes(batch, ref, prm)   the error-profile rows of an aligned batch

`ref` is the nanosim_amd.model.Reference the batch was drawn from (the .ref of a metagenome / transcriptome reference), `prm` the
ns_params.  The second record pass of -k (MAT_HP_FINAL) reads an edit list that is no part of an oracle batch: batches with kmer_bias
are refused.  The record buffer and the error-profile buffer are allocated 64-byte aligned (ensure_all, H: ns_generate), so an
offset into them modulo 16 is the address modulo 16."""
import collections

import numpy as np

T_OUT = 2048            # M:650 output bytes of a first-pass tile (NS_TILE_CHUNKS = 2 chunks per lane)
DENSE_SEG = 4096        # H:1294 NS_DENSE_SEG
DENSE_TILE = 1024       # M:393 NS_DENSE_TILE
ERR_BUF_SMALL, ERR_BUF_LARGE, ERR_NAME = 5120, 8192, 256      # H:1869-1872
SPLICED_BASE = 1 << 56  # include/nanosim_amd.h: a piece copied from the splice arena, not from the reference
MIS, INS, DEL = 0, 1, 2
KIND_ALIGNED, KIND_UNALIGNED = 0, 1

_AMB = np.ones(256, dtype=bool)                       # normalise_base (ns_device.h:365): everything but ACGT / acgt carries bit 7 on the device
for _c in b"ACGTacgt":
    _AMB[_c] = False


def _events(batch, p):
    """(first output offset, letters, type, length, segment position, resume position) of the events of piece p, as int64 arrays"""
    e = batch["events"][int(p["ev_off"]):int(p["ev_off"]) + int(p["n_ev"])]
    info = e["info"].astype(np.int64)
    ln, ty, sh = info & 0xFFF, (info >> 12) & 3, (info >> 14) - 131072
    pos = e["pos"].astype(np.int64)
    return pos + sh, np.where(ty == DEL, 0, ln), ty, ln, pos, pos + np.where(ty == INS, 0, ln)      # M:252-256


def _seq_line(batch, r):
    """offset of the sequence line of read r in the record image, and the length of the read name (H:1173: rec_off + name_len + 2)"""
    ro = int(r["rec_off"])
    rec = batch["records"]
    nl = int(np.flatnonzero(rec[ro:ro + 8192] == 10)[0]) - 1
    return ro + nl + 2, nl


class _Span:
    """the reference under a piece: ambiguity flags by segment position (load_piece, M:300-312; circular wrap, M:277-281)"""

    def __init__(self, ref, p):
        self.pos, self.ref_len = int(p["pos"]), int(p["ref_len"])
        self.spliced = int(p["ref_gpos"]) >= SPLICED_BASE
        c = int(p["chrom"])
        self.base = int(ref.chrom_off[c])
        self.chrom_len = (1 << 62) if self.spliced else int(ref.chrom_off[c + 1]) - self.base
        self.circular = bool(ref.circular[c]) and not self.spliced
        self.wraps = self.pos + self.ref_len > self.chrom_len                                  # M:699
        self.lin = self.chrom_len - self.pos                                                   # M:401, M:700 (wrap_at)
        self._ref = ref
        self._amb = None

    def amb(self, x):
        """ambiguity flag of segment positions x (array; positions outside the segment read as plain)"""
        x = np.asarray(x, dtype=np.int64)
        if self.spliced:
            return np.zeros(x.shape, dtype=bool)
        if self._amb is None:
            idx = (self.pos + np.arange(self.ref_len, dtype=np.int64)) % self.chrom_len
            self._amb = _AMB[self._ref.bases[self.base + idx]]
        ok = (x >= 0) & (x < self.ref_len)
        out = np.zeros(x.shape, dtype=bool)
        out[ok] = self._amb[x[ok]]
        return out

    def any_amb(self):
        return bool(self.amb(np.arange(self.ref_len)).any()) if self.ref_len else False


def _window_amb(span, x0, width):
    """per start position x0[i]: any ambiguity code in [x0[i], x0[i] + width[i])  (width: scalar or array)"""
    x0 = np.asarray(x0, dtype=np.int64)
    width = np.broadcast_to(np.asarray(width, dtype=np.int64), x0.shape)
    if not len(x0) or span.spliced or not span.any_amb():
        return np.zeros(x0.shape, dtype=bool)
    cs = np.concatenate([[0], np.cumsum(span.amb(np.arange(span.ref_len)))])
    lo, hi = np.clip(x0, 0, span.ref_len), np.clip(x0 + width, 0, span.ref_len)
    return cs[hi] > cs[lo]


# ---- the tile loop of materialise_piece ---------------------------------------------------------------------------------------------
def piece_tiles(os_, pl, ty, rp, out_len, phi, span):
    """The tiles materialise_piece cuts a piece into (M:708-743, 779-796), as dicts: M0, M1, A0, jb (events in front of the tile), cnt
    (events the tile takes), queued (None, or why the tile goes to the slow queue: "stuck" = 64 events at one offset, "origin"),
    cut (None, "chunk" = ended early on a chunk boundary, "inside" = inside a chunk), L0 (index of the event in force at M0, -1: none)"""
    n = len(os_)
    M0, jb, L0 = 0, 0, -1
    while M0 < out_len:
        A0 = M0 - ((M0 - phi) & 15)                                                            # M:709
        M1 = min(A0 + T_OUT, out_len)                                                          # M:710
        cut = None
        if jb + 63 < n and int(os_[jb + 63]) < M1:                                             # M:717-719
            o63 = int(os_[jb + 63])
            c = A0 + ((o63 - A0) & ~15)                                                        # M:720
            if c - M0 > 0:                                                                     # M:721
                M1, cut = c, "chunk"
            else:
                M1, cut = o63, "inside"
        if M1 <= M0:                                                                           # M:726
            M1 = min(M0 + T_OUT, out_len)                                                      # M:728
            j2 = jb + int(np.searchsorted(os_[jb:], M1, side="left"))                          # M:730
            yield dict(M0=M0, M1=M1, A0=A0, jb=jb, cnt=j2 - jb, queued="stuck", cut=cut, L0=L0)
            if j2 > jb:
                L0 = j2 - 1                                                                    # M:732-737
            jb, M0 = j2, M1
            continue
        cnt = int(np.searchsorted(os_[jb:min(jb + 64, n)], M1, side="left"))                   # M:724-725
        last = jb + cnt - 1 if cnt else L0                                                     # M:770-777
        queued = None
        if span.wraps:                                                                         # M:780-788
            if L0 < 0:
                x0 = M0                                                                        # (synthetic start: copy from 0)
            else:
                d0 = M0 - int(os_[L0])
                x0 = int(rp[L0]) if (d0 < int(pl[L0]) and int(ty[L0]) == INS) else int(rp[L0]) + d0 - int(pl[L0])
            if last < 0:
                x1 = M1
            else:
                dl = M1 - int(os_[last])
                x1 = int(rp[last]) if dl <= int(pl[last]) else int(rp[last]) + dl - int(pl[last])
            x1 = max(x1, x0)
            queued = "beyond" if x0 >= span.lin else "origin" if x1 > span.lin else "before"
        yield dict(M0=M0, M1=M1, A0=A0, jb=jb, cnt=cnt, queued="origin" if queued == "origin" else None, cut=cut, L0=L0,
                   origin=queued)
        L0 = last
        jb, M0 = jb + cnt, M1


def record_pieces(batch, prm):
    """(read, sequence-line offset, piece, output offset of the piece in the read, phi) of every piece k_materialise<., MAT_REF> takes"""
    if int(prm.kmer_bias):
        raise ValueError("the record census covers the first pass without -k only")
    if int(prm.kind) == KIND_UNALIGNED:
        raise ValueError("unaligned batches take k_materialise_dense: dense_classes")
    pieces = batch["pieces"]
    for r in batch["reads"]:
        if int(r["flags"]):
            continue
        seq, _ = _seq_line(batch, r)
        pq = int(r["head"])                                                                    # H:1235
        for pi in range(int(r["piece_off"]), int(r["piece_off"]) + int(r["n_pieces"])):
            p = pieces[pi]
            # M:702: the offsets m = phi (mod 16) of the piece start an aligned 16-byte group of the destination
            phi = ((seq + int(r["seq_len"]) - pq) & 15) if int(r["reversed"]) else ((-(seq + pq)) & 15)
            yield r, seq, p, pq, phi
            pq += int(p["out_len"])


def record_classes(batch, ref, prm):
    C = collections.Counter()
    for k in ("tile_cut_inside_chunk", "tile_64_events_at_one_offset", "class_word_carry", "tile_mid_piece_chunk0_before_M0",
              "max_events_in_chunk", "max_events_in_chunk_gap"):
        C[k] = 0
    for r, seq, p, pq, phi in record_pieces(batch, prm):
        out_len, kind = int(p["out_len"]), int(p["kind"])
        os_, pl, ty, ln, epos, rp = _events(batch, p)
        n = len(os_)
        s1 = os_ + pl
        span = _Span(ref, p)
        rev = int(r["reversed"])
        C["pieces"] += 1
        C["piece_gap"] += kind != 0                          # H:1237: the gaps of a chimeric read take the same tile loop (sid NS_GAP_SEG + ., M:310)
        C["phi_%d" % phi] += 1                               # M:702
        C["strand_reverse" if rev else "strand_forward"] += 1         # M:135 prep_chunk
        C["piece_shorter_than_16"] += out_len < 16           # M:744 nc == 1, front- and back-partial chunk at once (M:945, M:83)
        C["piece_no_event"] += n == 0                        # M:704 no lane loads an event; every tile has cnt == 0
        C["piece_wraps_origin"] += span.wraps                # M:699
        C["event_at_piece_end"] += int((os_ >= out_len).sum())   # M:724 a trailing deletion: taken by no tile
        # the piece's chunk grid: chunk k covers its positions [16 k - g, 16 k - g + 16), g = -phi mod 16 (M:938)
        g = (-phi) & 15
        if n:
            per_chunk = np.bincount((os_ + g) >> 4)
            key = "max_events_in_chunk_gap" if kind else "max_events_in_chunk"
            C[key] = max(C[key], int(per_chunk.max()))
        # ambiguity codes under copied bytes, by chunk of the piece (resolve16 on a chunk-lane sub-run M:933 / an event sub-run M:911)
        if not span.spliced and span.any_amb():
            st = np.concatenate([[0], s1])
            en = np.concatenate([os_, [out_len]])
            x0 = np.concatenate([[0], rp])
            cl = np.maximum(en - st, 0)
            tot = int(cl.sum())
            if tot:
                first = np.repeat(np.cumsum(cl) - cl, cl)
                k = np.arange(tot) - first
                m = np.repeat(st, cl) + k
                a = span.amb(np.repeat(x0, cl) + k)
                C["iupac_under_copy_chunks"] += len(np.unique((m[a] + g) >> 4))
        mis = ty == MIS
        amb_sub = _window_amb(span, epos, np.where(mis, pl, 0))          # codes under the substituted bases themselves (M:897 resolve_base)
        amb_sub8 = _window_amb(span, epos, np.where(mis, 8, 0))          # codes in the 8 bytes the fast path loads (M:845-846)
        prev_cont = False
        for t in piece_tiles(os_, pl, ty, rp, out_len, phi, span):
            M0, M1, A0, jb, cnt, L0 = t["M0"], t["M1"], t["A0"], t["jb"], t["cnt"], t["L0"]
            C["tiles"] += 1
            C["tile_cut_on_chunk_boundary"] += t["cut"] == "chunk"                             # M:721 cut > M0
            C["tile_cut_inside_chunk"] += t["cut"] == "inside"                                 # M:721 M1 = os63
            if t["queued"] == "stuck":
                C["tile_64_events_at_one_offset"] += 1                                         # M:726-743
                prev_cont = False
                continue
            if span.wraps:
                C["tile_%s_origin" % ("straddles" if t["origin"] == "origin" else t["origin"])] += 1     # M:786 / M:787 / neither
            if t["queued"]:
                prev_cont = False
                continue                                                                       # M:789-796 slow queue
            C["tile_first_A0_negative"] += A0 < 0                                              # M:709 (wrapped), M:923 ci == 0
            C["tile_mid_piece_chunk0_before_M0"] += M0 > 0 and A0 < M0                          # M:810, M:923 ci == 0 behind a cut inside a chunk
            C["tile_cnt_0" if cnt == 0 else "tile_cnt_63" if cnt == 63 else "tile_cnt_1_62"] += 1       # M:725, M:771
            nc = (M1 - A0 + 15) >> 4                                                           # M:744 (never above 128: M1 <= A0 + T_OUT)
            C["tile_nc_above_64"] += nc > 64                                                   # M:804 second chunk of a lane
            C["tile_nc_128"] += nc == 128
            C["tile_last_chunk_partial"] += ((M1 - A0) & 15) != 0                              # M:923 hi_m < c0 + 16, store16 count < 16
            C["class_word_carry"] += M1 < out_len and ((M1 - A0) & 15) != 0                    # M:954 cls_carry != 0 (FASTQ batches read it, M:940)
            C["tile_L0_%s" % ("start" if L0 < 0 else ("mis", "ins", "del")[int(ty[L0])])] += 1   # M:697, M:750 the event in force at M0
            cont = L0 >= 0 and int(s1[L0]) > M0                                                # M:834 lane 63 continues a payload
            C["payload_continued"] += cont
            C["payload_continued_twice"] += cont and prev_cont                                  # ... of the same event as in the tile before
            C["payload_continued_beyond_tile"] += cont and int(s1[L0]) > M1
            prev_cont = cont and int(s1[L0]) > M1
            j = slice(jb, jb + cnt)
            o, l, e_s1, e_ty = os_[j], pl[j], s1[j], ty[j]
            has = l > 0
            inside = e_s1 <= M1
            fast = has & (l <= 8) & inside & (not span.wraps) & ~(amb_sub8[j] & (e_ty == MIS))  # M:843-846
            C["letters_1_7"] += int((fast & (l < 8)).sum())                                    # M:872 keep mask
            for a in range(4):
                C["letters_8_at_%d" % a] += int((fast & (l == 8) & (((o - A0) & 3) == a)).sum())    # M:874-878 the third dword OR
            slow = has & ~fast                                                                 # M:880
            C["letters_9_16"] += int((slow & (l > 8) & (l <= 16)).sum())
            C["letters_above_16"] += int((slow & (l > 16)).sum())                              # M:885 a second payload_word
            C["letters_cut_by_tile_end"] += int((has & ~inside).sum())                         # M:882 i_hi = M1 - b_os
            C["letters_slow_piece_wraps"] += int((has & (l <= 8) & inside).sum()) if span.wraps else 0
            C["iupac_under_substitution"] += int((amb_sub[j] & (e_ty == MIS)).sum())           # M:897
            C["iupac_next_to_substitution"] += int((amb_sub8[j] & ~amb_sub[j] & (e_ty == MIS) & (l <= 8) & inside).sum())   # M:846 only
            C["event_at_chunk_start"] += int(((o > M0) & (((o - A0) & 15) == 0)).sum())        # M:747 ekey = the chunk itself
            C["event_at_tile_start"] += int((o == M0).sum())                                   # M:747 os <= M0
            # 3b (M:825-830): the sub-run behind the event's letters; empty when the letters end on a chunk end (then the chunk lane has it)
            ekey = np.where(o <= M0, 0, (o - A0 + 15) >> 4)
            c = (e_s1 - A0) >> 4
            nxt = np.concatenate([os_[jb + 1:jb + cnt], [1 << 62]]) if cnt else o             # M:763 (the last taken event: none)
            en = np.minimum(nxt, np.minimum(A0 + 16 * c + 16, M1))
            sub = (en > e_s1) & (ekey > c)
            C["event_subrun"] += int(sub.sum())
            C["event_subrun_empty"] += int((~sub).sum())
            C["letters_end_at_chunk_end"] += int((has & (((e_s1 - A0) & 15) == 0) & inside).sum())
            # 3a (M:806-817): per chunk, the event in force at its first byte and the sub-run copied under it
            ci = np.arange(nc)
            cs = A0 + 16 * ci
            cend = np.minimum(cs + 16, M1)
            incl = np.searchsorted(ekey, ci, side="right")                                     # events sorted in front of the chunk (M:764-768)
            ex = np.concatenate([[int(s1[L0]) if L0 >= 0 else 0], e_s1])[incl]                  # M:750-752 ent[].x
            C["chunk_wholly_under_letters"] += int((ex >= cend).sum())                         # M:814 en <= st: no load
            echunk = np.where(o < A0 + 16, 0, (o - A0) >> 4) if cnt else np.zeros(0, dtype=np.int64)
            C["chunk_without_event"] += nc - len(np.unique(echunk))                            # M:767 the chunk inherits hist through the prefix maximum
            C["chunks"] += nc
    return dict(C)


# ---- dense_piece ---------------------------------------------------------------------------------------------------------------------
def dense_classes(batch, ref, prm):
    if int(prm.kind) != KIND_UNALIGNED:
        raise ValueError("only batches of unaligned reads take k_materialise_dense (launch_materialise, H:2656)")
    C = collections.Counter()
    for k in ("stretch_cuts_piece_off_16", "item_across_origin", "item_near_origin"):
        C[k] = 0
    pieces = batch["pieces"]
    for r in batch["reads"]:
        if int(r["flags"]):
            continue
        C["reads"] += 1
        C["read_shorter_than_16"] += int(r["seq_len"]) < 16                                    # M:506 one partial store per read
        C["read_several_stretches"] += int(r["seq_len"]) > DENSE_SEG                           # H:1302
        q = int(r["head"])
        for pi in range(int(r["piece_off"]), int(r["piece_off"]) + int(r["n_pieces"])):
            p = pieces[pi]
            out_len = int(p["out_len"])
            os_, pl, ty, ln, epos, rp = _events(batch, p)
            n = len(os_)
            span = _Span(ref, p)
            C["piece_no_event"] += n == 0                                                      # M:399 one item
            p_lo = q - int(r["head"])                                                          # H:1322
            it_os = np.concatenate([[0], os_])                                                 # item 0: the stretch in front of the first event
            it_pl = np.concatenate([[0], pl])
            it_ty = np.concatenate([[3], ty])
            it_rp = np.concatenate([[0], rp])
            it_pos = np.concatenate([[0], epos])
            it_nx = np.concatenate([os_, [out_len]])
            n_seg = max(1, -(-int(r["seq_len"]) // DENSE_SEG))
            for seg in range(n_seg):
                s_lo, s_hi = seg * DENSE_SEG, (seg + 1) * DENSE_SEG
                if not (p_lo + out_len > s_lo and p_lo < s_hi):                                # H:1323
                    continue
                m_lo, m_hi = max(s_lo, p_lo) - p_lo, min(s_hi, p_lo + out_len) - p_lo
                C["stretches"] += 1
                if m_lo & 15:                                                                  # M:398 slow_piece_range takes the stretch
                    C["stretch_cuts_piece_off_16"] += 1
                    continue
                for M0 in range(m_lo, m_hi, DENSE_TILE):                                       # M:404
                    M1 = min(M0 + DENSE_TILE, m_hi)
                    C["tiles"] += 1
                    C["tile_partial_last_chunk"] += ((M1 - M0) & 15) != 0                      # M:506
                    a0 = int(np.searchsorted(it_nx, M0, side="right"))                         # first item with nxt > M0
                    a1 = int(np.searchsorted(it_os, M1, side="left"))                          # items with os < M1
                    s = slice(a0, a1)
                    o, l, t_, nx = it_os[s], it_pl[s], it_ty[s], it_nx[s]
                    lo, hi = np.maximum(o, M0), np.minimum(nx, M1)
                    act = lo < hi                                                              # M:421
                    jb = int(np.searchsorted(it_os, M0, side="right")) - 1                     # M:403, M:501 item in force at the tile start
                    C["tile_more_than_64_items"] += a1 - jb > 64                               # M:407 a second round of the item loop
                    n_let = np.where(act, np.minimum(l, hi - o), 0)                            # M:422
                    c_lo = np.maximum(lo, o + l)                                               # M:423
                    cn = np.where(act & (c_lo < hi), hi - c_lo, 0)                             # M:424
                    x0 = it_rp[s] + (c_lo - o - l)                                             # M:425
                    notins = t_ != INS
                    sub_pos = it_pos[s]
                    fast_l = (n_let > 0) & (o >= M0) & (~notins | (sub_pos + n_let <= span.lin))   # M:429
                    C["letters_cut_by_tile_start"] += int(((n_let > 0) & (o < M0)).sum())       # M:429 os < M0 -> M:478 per-byte walk
                    C["letters_cut_by_tile_end"] += int((act & (l > hi - o) & (hi == M1)).sum())   # M:422 n_let < pl
                    C["letters_above_4"] += int((fast_l & (n_let > 4)).sum())                  # M:445 more than one group
                    C["letters_above_16"] += int((fast_l & (n_let > 16)).sum())                # M:448 a second payload_word
                    C["substitution_across_origin"] += int(((n_let > 0) & notins & (o >= M0) & (sub_pos + n_let > span.lin)).sum())
                    C["copy_above_16"] += int((cn > 16).sum())                                 # M:430 -> M:491 per-byte walk
                    C["copy_cut_by_tile_end"] += int(((cn > 0) & (nx > M1)).sum())             # M:420 hi = M1
                    C["copy_cut_by_tile_start"] += int(((cn > 0) & (o + l < M0)).sum())        # M:420 lo = M0
                    C["copy_1_16"] += int(((cn > 0) & (cn <= 16)).sum())                       # M:475 lds_put_bytes
                    amb_c = _window_amb(span, x0, cn)
                    amb_16 = _window_amb(span, x0, np.where((cn > 0) & (cn <= 16) & (x0 + 16 <= span.lin), 16, 0))
                    C["iupac_under_copy"] += int(amb_c.sum())                                  # M:433 -> M:494 resolve_base
                    C["iupac_next_to_copy"] += int((amb_16 & ~amb_c).sum())                    # M:433 only: a code in the 16 bytes loaded, not copied
                    amb_s = _window_amb(span, sub_pos, np.where(notins & (t_ != 3), n_let, 0))
                    C["iupac_under_substitution"] += int(amb_s.sum())                          # M:452 / M:486
                    if span.circular:
                        C["item_near_origin"] += int(((cn > 0) & (x0 + 16 > span.lin) & (x0 + cn <= span.lin)).sum())   # M:430 within 16 bases of it
                        C["item_across_origin"] += int(((cn > 0) & (x0 < span.lin) & (x0 + cn > span.lin)).sum())      # M:279 wrap inside the copy
                        C["item_beyond_origin"] += int(((cn > 0) & (x0 >= span.lin)).sum())
            q += out_len
    return dict(C)


# ---- k_errlog ------------------------------------------------------------------------------------------------------------------------
def _digits(x):
    return np.where(x == 0, 1, np.floor(np.log10(np.maximum(x, 1))).astype(np.int64) + 1)


def errlog_rows(batch, prm):
    """per read with rows: (read index, name length, [(piece, row lengths in the order they are written = last event first)])"""
    if int(prm.kmer_bias):
        raise ValueError("with -k the rows are those of the filtered event list: not covered")
    pieces = batch["pieces"]
    for ri, r in enumerate(batch["reads"]):
        if int(r["flags"]):
            continue
        _, nl = _seq_line(batch, r)
        out = []
        for pi in range(int(r["piece_off"]), int(r["piece_off"]) + int(r["n_pieces"]), 2):     # H:1902
            p = pieces[pi]
            if int(p["kind"]):
                continue                                                                       # H:1835 gaps have no rows
            os_, pl, ty, ln, epos, rp = _events(batch, p)
            rows = nl + _digits(epos) + _digits(ln) + 2 * ln + 9                               # H:1839, H:1913
            out.append((p, rows[::-1]))
        yield ri, nl, out


def errlog_buf(batch):
    """the BUF ns_generate picks (H:3787-3789): from the batch's error-profile bytes per event (gap events included in the count)"""
    rows = len(batch["events"]) or 1
    return ERR_BUF_SMALL if (len(batch["errlog"]) // rows + 5) * 64 <= ERR_BUF_SMALL else ERR_BUF_LARGE


def errlog_classes(batch, ref, prm):
    C = collections.Counter()
    BUF = errlog_buf(batch)
    for k in ("row_name_no_whole_dword", "name_above_256", "block_above_buf", "blocks_5120", "blocks_8192"):
        C[k] = 0
    base = 0
    for ri, nl, plist in errlog_rows(batch, prm):
        C["reads"] += 1
        C["name_above_256"] += nl > ERR_NAME                                                   # H:1887 name_in_lds false
        C["read_several_aligned_pieces"] += len(plist) > 1                                     # H:1902
        for p, rows in plist:
            n = len(rows)
            C["piece_no_event"] += n == 0                                                      # H:1907 no iteration
            C["n_ev_multiple_of_64"] += n > 0 and n % 64 == 0                                  # H:1910 every lane active in the last block
            os_, pl, ty, ln, epos, rp = (a[::-1] for a in _events(batch, p))
            span = _Span(ref, p)
            need_ref = ty != INS                                                               # H:1935
            inside = span.pos + epos + 16 <= span.chrom_len                                    # H:1936
            amb = _window_amb(span, epos, np.where(need_ref, ln, 0))
            C["len_1_16"] += int((ln <= 16).sum())                                             # H:1939
            C["len_above_16"] += int((ln > 16).sum())                                          # H:1971 per-byte loop, a second payload_word H:1974
            for k in np.unique(ln[need_ref & inside & (ln <= 16)]):
                C["len_q%d_r%d" % (k >> 2, k & 3)] += int((need_ref & inside & (ln == k)).sum())    # H:1941-1944 the ambiguity mask
            C["iupac_under_event"] += int(amb.sum())                                           # H:1945 -> H:1978
            C["window_leaves_%s" % ("circular" if span.circular else "linear")] += int((need_ref & ~inside).sum())   # H:1936 inside false
            C["event_across_origin"] += int((need_ref & (span.pos + epos < span.chrom_len) & (span.pos + epos + ln > span.chrom_len)).sum())
            for d in range(1, 8):
                C["pos_digits_%d" % d] += int((_digits(epos) == d).sum())                      # put_dec_p, H:1923
            for d in range(1, 5):
                C["len_digits_%d" % d] += int((_digits(ln) == d).sum())                        # H:1926
            for j0 in range(0, n, 64):                                                         # H:1907
                blk = rows[j0:j0 + 64]
                total = int(blk.sum())                                                         # H:1916
                C["blocks"] += 1
                C["blocks_%d" % BUF] += 1                                                      # H:3788 the kernel the batch's average row picks
                C["block_above_buf"] += total > BUF
                staged = nl <= ERR_NAME and total <= BUF                                       # H:1917
                if staged:
                    C["blocks_staged"] += 1
                    mis = base & 15                                                            # H:1989
                    C["mis_%d" % mis] += 1
                    o = mis + np.concatenate([[0], np.cumsum(blk)[:-1]])                       # H:1991
                    al = o & 3                                                                 # H:1992
                    for a in range(4):
                        C["al_%d" % a] += int((al == a).sum())
                    C["row_name_no_whole_dword"] += int((((al + nl) >> 2) <= (al != 0)).sum())     # H:1999 d1 > d0 false
                else:
                    C["blocks_unstaged"] += 1
                    C["rows_unstaged_nl_%d" % (nl & 15)] += len(blk)                           # H:2033-2035
                    C["rows_unstaged_name_below_16"] += len(blk) if nl < 16 else 0             # H:2036
                base += total                                                                  # H:2040
    C["predicted_bytes"] = base
    return dict(C)
