// ns_chimeric.h — training side, chimeric reads ("Chimeric reads: the split-alignment choice"): what
// primary_and_unaligned_chimeric of src/get_primary_sam.py (G:220-478) decides for every primary alignment that carries an SA:Z tag —
// which of its split alignments belong to the read, in which order, and which gaps lie between them.  G: = src/get_primary_sam.py of
// bcgsc/NanoSim v3.2.2.
//
// Per CIGAR (chim_scan_cigar, one CIGAR per thread in k_chim_scan), in one of two readings:
//   CHIM_PARSER  cigar_parser (G:16-31), the figures of an SA entry and of a supplementary / secondary record:
//                  qstart = the count of the first op when that op is S or H, else 0;  qlen = M + I;  rlen = M + D;  qend = qstart + qlen.
//                Only M, I and D are summed: the reference's regular expression `(\d+)(\w)` ignores X, N, P and every later clip, and it
//                does not see `=` at all (`=` is no \w) — an `=` op adds nothing to either sum.  Kept, as is what follows from it for the
//                FIRST item: an `=` op whose count has two digits or more still leaves an item (`10=` matches as count `1`, op `0`), which
//                is no clip, so qstart is 0 behind it; an `=` op with a one-digit count leaves none, and the op behind it is the first.
//   CHIM_PYSAM   what pysam states for the primary alignment (G:280, 291-293):
//                  qstart = query_alignment_start = the S ops among the leading clips (H is not in the sequence);
//                  qlen = query_alignment_length = M + I + `=` + X;  qend = query_alignment_end = qstart + qlen;
//                  rlen = reference_end - reference_start = M + D + N + `=` + X.
// A CIGAR is BAD — all figures 0 — when it is empty, holds a byte that is neither a digit nor one of MIDNSHP=X, has an op without a count
// (or a count without an op), or has a sum beyond 32 bits (qend or rlen).
//
// Per read (chim_select_read, one read per thread in k_chim_select): entry 0 is the primary alignment, entries 1 .. n its SA entries in
// tag order.  score = qlen - NM (signed), reference interval = (ref_start, ref_start + rlen), ref_start = the tag's position - 1.
//   grouping  (G:297-319) every SA entry is offered to every list that exists when its turn comes, in order, and is appended to EVERY list
//             it is compatible with — an entry can sit in several lists —; when no list takes it, it opens a new one.  List 0 starts
//             with the primary.
//   compatible (not_overlap, G:34-41) with a list = with each of its members: the query intervals do not overlap, and neither do the
//             reference intervals of members on the same reference; two intervals overlap when a.start < b.end - 10 and
//             a.end - 10 > b.start, exactly as written at G:38 (signed: an end below 10 makes the right side negative).
//   winner    (G:321-323) the first list with the largest score.
//   alone     (G:325-337) a winner of one piece whose qstart is not the primary's: the read is not chimeric.  The primary record is kept
//             alone, no gap is recorded, pos_strand counts the primary's direction.
//   order     (G:338-341) otherwise the pieces are sorted by (qstart, qend), stably; reference interval and name follow, the direction
//             list does NOT (seg["direction"] is never permuted).
//   gaps      (G:357-368) between consecutive pieces max(0, qstart_i - qend_{i-1}), except where both lie on the same reference and their
//             edges (edge_checker = len_edge of ns_read_len.h, with the piece's own rlen) are opposite: start edge then end edge, or
//             the reverse — the two ends of a circular reference.  A recorded gap adds 1 to
//             species_count[species of the previous piece][same species ? 0 : 1].
//   pos_strand (G:369-372, 382-384) +1 for EVERY piece whose qstart equals the primary's when the primary is forward (the reference
//             tells the primary by that equality, not by identity: such a piece is also written as the primary record); when no piece
//             has it, +1 if the direction of the list's FIRST-ADDED entry is `+`.
// Membership of an entry in a list is a bit mask over the read's entries: list j owns words j * W .. j * W + W - 1 of the read's
// workspace, W = ceil((n + 1) / 64), and there are at most n + 1 lists — (n + 1) * W 64-bit words, no cap on n.  A list's score and its
// first-added entry are recomputed from its mask (entries join in index order: the first-added one is the lowest bit).
// The code below compiles for the device (k_chim_scan, k_chim_select in ns_train.h) and, unchanged, for the host (tests/chimeric_host.cpp).
#pragma once
#include <stdint.h>
#include "ns_read_len.h"

enum { CHIM_PARSER = 0, CHIM_PYSAM = 1 };
enum { CHIM_POS_STRAND = 1, CHIM_ALONE = 2, CHIM_HAS_SA = 4 };        // ns_chim_read.flags (NS_CHIM_* of include/nanosim_amd.h)
#define NS_CHIM_OVERLAP_BASE 10                                        // overlap_base (G:34)
#define NS_CHIM_NO_GAP_V (-1ll)                                        // NS_CHIM_NO_GAP

struct ChimFigures { uint32_t qstart, qend, qlen, rlen; };             // = ns_chim_ent
struct ChimPiece { uint32_t entry, is_primary; int64_t gap; };         // = ns_chim_piece
struct ChimTotals { uint64_t n_gaps, pos_strand; };

NS_CSH uint64_t chim_mask_words(uint64_t n_entries) { return (n_entries + 63u) >> 6; }
NS_CSH uint64_t chim_ws_words(uint64_t n_entries) { return n_entries * chim_mask_words(n_entries); }

template <class S>
NS_CSH bool chim_scan_cigar(S &cg, uint64_t cn, int how, ChimFigures &F) {
    F.qstart = F.qend = F.qlen = F.rlen = 0;
    if (!cn) return false;
    uint64_t qstart = 0, qlen = 0, rlen = 0;
    bool leading = true;                                   // CHIM_PARSER: no item yet; CHIM_PYSAM: still inside the leading clips
    uint64_t i = 0;
    while (i < cn) {
        uint64_t n;
        const uint64_t at = i;
        if (!sam_number(cg, cn, i, n) || i >= cn) return false;     // an op without a count, a byte that is no op, a count without an op
        const uint64_t digits = i - at;
        const uint8_t op = cg[i++];
        if (op != 'M' && op != 'I' && op != 'D' && op != 'N' && op != 'S' && op != 'H' && op != 'P' && op != '=' && op != 'X') return false;
        if (how == CHIM_PARSER) {
            if (op == '=') { if (digits > 1u) leading = false; continue; }     // (`10=`: the item `1`,`0`; `5=`: no item)
            if (leading) { leading = false; if (op == 'S' || op == 'H') qstart = n; }
            if (op == 'M') { qlen += n; rlen += n; }
            else if (op == 'I') qlen += n;
            else if (op == 'D') rlen += n;
        } else {
            if (leading && op == 'S') qstart += n;
            else if (op != 'H') leading = false;
            if (op == 'M' || op == '=' || op == 'X') { qlen += n; rlen += n; }
            else if (op == 'I') qlen += n;
            else if (op == 'D' || op == 'N') rlen += n;
        }
        // (sam_number saturates at 2^40 and the walk ends as soon as a sum passes 2^32: no 64-bit sum can wrap)
        if (qstart + qlen > 0xffffffffull || rlen > 0xffffffffull) return false;
    }
    F.qstart = (uint32_t)qstart; F.qlen = (uint32_t)qlen; F.rlen = (uint32_t)rlen; F.qend = (uint32_t)(qstart + qlen);
    return true;
}

// not_overlap's condition for one pair (G:38): interval a against member b
NS_CSH bool chim_overlap(int64_t a0, int64_t a1, int64_t b0, int64_t b1) {
    return a0 < b1 - NS_CHIM_OVERLAP_BASE && a1 - NS_CHIM_OVERLAP_BASE > b0;
}

// The choice for one read.  n_ent: its entries (>= 1); ent / ref_id / ref_start / nm / reverse: per entry, entry 0 the primary (ent[0]
// in the CHIM_PYSAM reading); ref_total / species: per reference; ws: chim_ws_words(n_ent) words, contents undefined; pieces: room for
// n_ent pieces; species_count: [n_species][2], added to through add(p, v) (an atomic on the device); T: the read's own contribution.
// returns n_pieces; flags: CHIM_*
template <class Add>
NS_CSH uint32_t chim_select_read(uint64_t n_ent, const ChimFigures *ent, const uint32_t *ref_id, const uint64_t *ref_start, const uint32_t *nm,
                                 const uint8_t *reverse, const uint64_t *ref_total, const uint32_t *species, uint64_t *ws, ChimPiece *pieces,
                                 unsigned long long *species_count, Add &add, ChimTotals &T, uint32_t &flags) {
    T.n_gaps = 0; T.pos_strand = 0;
    const bool primary_forward = reverse[0] == 0;
    const uint32_t primary_qstart = ent[0].qstart;
    if (n_ent == 1u) {                                     // no SA tag (G:387-395)
        pieces[0] = ChimPiece{0u, 1u, NS_CHIM_NO_GAP_V};
        T.pos_strand = primary_forward ? 1u : 0u;
        flags = primary_forward ? (uint32_t)CHIM_POS_STRAND : 0u;
        return 1u;
    }
    flags = CHIM_HAS_SA;
    const uint64_t W = chim_mask_words(n_ent);
    uint64_t n_lists = 1;
    for (uint64_t w = 0; w < W; ++w) ws[w] = 0;
    ws[0] = 1ull;
    for (uint64_t e = 1; e < n_ent; ++e) {
        const ChimFigures E = ent[e];
        const int64_t q0 = (int64_t)E.qstart, q1 = (int64_t)E.qend, r0 = (int64_t)ref_start[e], r1 = r0 + (int64_t)E.rlen;
        const uint32_t rid = ref_id[e];
        bool added = false;
        for (uint64_t l = 0; l < n_lists; ++l) {
            uint64_t *mask = ws + l * W;
            bool ok = true;
            for (uint64_t w = 0; w < W && ok; ++w) {
                uint64_t bits = mask[w];
                while (bits) {
                    const uint64_t m = (w << 6) + (uint64_t)__builtin_ctzll(bits);
                    bits &= bits - 1u;
                    const ChimFigures M = ent[m];
                    const int64_t m0 = (int64_t)ref_start[m];
                    if (chim_overlap(q0, q1, (int64_t)M.qstart, (int64_t)M.qend) ||
                        (ref_id[m] == rid && chim_overlap(r0, r1, m0, m0 + (int64_t)M.rlen))) { ok = false; break; }
                }
            }
            if (ok) { mask[e >> 6] |= 1ull << (e & 63u); added = true; }
        }
        if (!added) {
            uint64_t *mask = ws + n_lists * W;
            for (uint64_t w = 0; w < W; ++w) mask[w] = 0;
            mask[e >> 6] = 1ull << (e & 63u);
            ++n_lists;
        }
    }
    // the first list with the largest score
    uint64_t best = 0; int64_t best_score = 0;
    for (uint64_t l = 0; l < n_lists; ++l) {
        const uint64_t *mask = ws + l * W;
        int64_t score = 0;
        for (uint64_t w = 0; w < W; ++w) {
            uint64_t bits = mask[w];
            while (bits) {
                const uint64_t m = (w << 6) + (uint64_t)__builtin_ctzll(bits);
                bits &= bits - 1u;
                score += (int64_t)ent[m].qlen - (int64_t)nm[m];
            }
        }
        if (l == 0 || score > best_score) { best = l; best_score = score; }
    }
    const uint64_t *win = ws + best * W;
    uint32_t k = 0;
    uint64_t first_added = 0;
    for (uint64_t w = 0; w < W; ++w) {
        uint64_t bits = win[w];
        while (bits) {
            const uint64_t m = (w << 6) + (uint64_t)__builtin_ctzll(bits);
            bits &= bits - 1u;
            if (!k) first_added = m;
            pieces[k++] = ChimPiece{(uint32_t)m, 0u, NS_CHIM_NO_GAP_V};
        }
    }
    if (k == 1u && ent[first_added].qstart != primary_qstart) {       // the only alignment picked is not the primary (G:325-337)
        pieces[0] = ChimPiece{0u, 1u, NS_CHIM_NO_GAP_V};
        T.pos_strand = primary_forward ? 1u : 0u;
        flags |= CHIM_ALONE | (primary_forward ? (uint32_t)CHIM_POS_STRAND : 0u);
        return 1u;
    }
    // stable insertion sort by (qstart, qend): the pieces stand in entry order, which is the order they were appended in
    for (uint32_t a = 1; a < k; ++a) {
        const ChimPiece P = pieces[a];
        const ChimFigures K = ent[P.entry];
        uint32_t b = a;
        while (b > 0) {
            const ChimFigures L = ent[pieces[b - 1u].entry];
            if (L.qstart < K.qstart || (L.qstart == K.qstart && L.qend <= K.qend)) break;
            pieces[b] = pieces[b - 1u];
            --b;
        }
        pieces[b] = P;
    }
    bool dir_added = false;
    uint32_t pre_edge = 0, pre_ref = 0, pre_species = 0, pre_qend = 0;
    for (uint32_t i = 0; i < k; ++i) {
        ChimPiece P = pieces[i];
        const ChimFigures E = ent[P.entry];
        const uint32_t rid = ref_id[P.entry];
        const uint32_t edge = len_edge(ref_start[P.entry], E.rlen, ref_total[rid]);
        const uint32_t sp = species[rid];
        if (i > 0) {
            const bool circular = rid == pre_ref && (((pre_edge & LEN_EDGE_START) && (edge & LEN_EDGE_END)) || ((pre_edge & LEN_EDGE_END) && (edge & LEN_EDGE_START)));
            if (!circular) {
                P.gap = E.qstart > pre_qend ? (int64_t)(E.qstart - pre_qend) : 0;
                T.n_gaps += 1u;
                add(&species_count[2u * pre_species + (sp == pre_species ? 0u : 1u)], 1ull);
            }
        }
        if (E.qstart == primary_qstart) {
            P.is_primary = 1u;
            dir_added = true;
            if (primary_forward) T.pos_strand += 1u;
        }
        pieces[i] = P;
        pre_edge = edge; pre_ref = rid; pre_species = sp; pre_qend = E.qend;
    }
    if (!dir_added && reverse[first_added] == 0) T.pos_strand += 1u;
    if (T.pos_strand) flags |= CHIM_POS_STRAND;
    return k;
}
