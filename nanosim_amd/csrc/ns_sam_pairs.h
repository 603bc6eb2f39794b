// ns_sam_pairs.h — training side, SAM input ("SAM input: the line pairs"): the two aligned lines of a SAM record — the
// reference line and the read line, `-` for gaps — from its CIGAR, its MD:Z tag and its SEQ.  This is what the reference gets from
// `samtools view | sam2pairwise` followed by src/pairwise2maf.py (P:38-82; src/read_analysis.py:200-204) before it trains the
// homopolymer-length model; the lines hold the M/=/X/I/D columns only (P:72, 76 cut the clips).  P: = src/pairwise2maf.py of
// bcgsc/NanoSim v3.2.2.
//
// Two phases.  SCAN (sam_scan_record, one record per thread in k_sam_scan): CIGAR and MD are walked together; the walk decides whether
// the record is valid, gives its four figures (head clip, tail clip, aligned reference length, aligned query length) and its number of
// columns, and writes the EXCEPTIONS in column order — insertion runs, deletion runs with the place of their letters in MD, mismatches
// with their letter.  Everything else is a column that shows the SEQ byte in both lines.  A record writes at most one exception per
// CIGAR op and one per `^` or mismatch letter of MD, so the list of record a begins at sam_exc_base(a): no counting pass.
// LINES (sam_cursor_at + sam_column; k_sam_lines): any column of the output is a function of the record's list and its SEQ — a search
// for the first exception that ends behind the column, then a walk forward.
//
// MD is `[0-9]+(([A-Za-z]|\^[A-Za-z]+)[0-9]+)*`: a number counts matching reference positions (it may be 0), insertions do not appear,
// a `^` run may feed several D ops (an I between them) and a D op may take the letters of two runs that a `0` separates.
// A record is BAD — zero columns, all figures 0 — when it holds an op outside MIDSH=X, an S that is not outermost (inside any H), an
// empty or `*` CIGAR or SEQ, a SEQ whose length is not the sum of its S/M/=/X/I ops, an M column that meets a `^` letter, a D column
// that meets anything else, an MD that ends early or has items left over, or 2^24 columns or more (the limit of ns_hp_histograms).
// The code below compiles for the device (k_sam_scan, k_sam_lines in ns_train.h) and, unchanged, for the host (tests/sam_pairs_host.cpp).
#pragma once
#include <stdint.h>
#include "ns_cs_hist.h"

enum { SAMX_INS = 0, SAMX_DEL = 1, SAMX_MIS = 2 };
#define NS_SAM_MAX_COLUMNS (1u << 24)
// one exception: `len` columns from column `col` on
struct SamExc {
    uint32_t col;
    uint32_t kind_len;                 // SAMX_* << 24 | len   (len < 2^24)
    uint32_t ndel;                     // deleted columns in front of `col`: a column c that is no deletion shows SEQ[head + c - ndel]
    uint32_t arg;                      // SAMX_DEL: where its letters begin in the record's MD; SAMX_MIS: the reference's letter
};
NS_CSH uint32_t sam_exc_kind(const SamExc &x) { return x.kind_len >> 24; }
NS_CSH uint32_t sam_exc_len(const SamExc &x) { return x.kind_len & 0xffffffu; }
// where the list of record a begins: ops <= CIGAR bytes / 2, letters and `^` <= MD bytes (+ a: the halves round down)
NS_CSH uint64_t sam_exc_base(const uint64_t *cigar_off, const uint64_t *md_off, uint64_t a) { return (cigar_off[a] >> 1) + md_off[a] + a; }

NS_CSH bool sam_is_digit(uint8_t c) { return c >= '0' && c <= '9'; }
NS_CSH bool sam_is_letter(uint8_t c) { return (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z'); }
// [0-9]+ at s[i]: false without a digit; values saturate far above any length a record can have
template <class S>
NS_CSH bool sam_number(S &s, uint64_t n, uint64_t &i, uint64_t &v) {
    if (i >= n || !sam_is_digit(s[i])) return false;
    v = 0;
    while (i < n && sam_is_digit(s[i])) { v = v * 10u + (uint64_t)(s[i] - '0'); if (v > (1ull << 40)) v = 1ull << 40; ++i; }
    return true;
}

struct SamFigures { uint32_t head, tail, ref_len, query_len, cols, n_exc; };

// The walk over one record.  cg / md: its CIGAR and MD bytes (cn, mn of them), sn: the length of its SEQ, seq_star: SEQ is `*`;
// exc: room for cn / 2 + mn + 1 exceptions.  false: the record is bad (F is all zero then).
template <class S>
NS_CSH bool sam_scan_record(S &cg, uint64_t cn, S &md, uint64_t mn, uint64_t sn, bool seq_star, SamExc *exc, SamFigures &F) {
    F.head = F.tail = F.ref_len = F.query_len = F.cols = F.n_exc = 0;
    if (!cn || !sn || seq_star) return false;
    uint64_t j = 0, left = 0;                  // the MD cursor: the next byte, what is left of the number in front of it
    bool in_del = false;                       // ... inside a `^` run: md[j] is its next letter
    if (!sam_number(md, mn, j, left)) return false;
    uint64_t col = 0, qi = 0, head = 0, tail = 0, ref = 0;     // columns so far, SEQ bytes of them, the clips, reference letters
    uint32_t n_exc = 0;
    int stage = 0;                             // 0 start, 1 leading H, 2 leading S, 3 columns, 4 trailing S, 5 trailing H
    uint64_t i = 0;
    while (i < cn) {
        uint64_t n;
        if (!sam_number(cg, cn, i, n) || i >= cn) return false;
        const uint8_t op = cg[i++];
        if (op == 'H') {
            if (stage == 1 || stage == 5) return false;
            stage = stage == 0 ? 1 : 5;
        } else if (op == 'S') {
            if (stage >= 4 || stage == 2) return false;
            if (stage < 2) { stage = 2; head = n; } else { stage = 4; tail = n; }
        } else if (op == 'M' || op == '=' || op == 'X') {
            if (stage > 3 || in_del) return false;                      // (an M column meets a `^` letter)
            stage = 3;
            while (n) {
                if (left) { const uint64_t t = left < n ? left : n; left -= t; n -= t; col += t; qi += t; ref += t; continue; }
                if (j >= mn) return false;                              // MD ends early
                const uint8_t c = md[j];
                if (!sam_is_letter(c)) return false;                    // `^`: a deletion where the CIGAR has none
                if (col >= NS_SAM_MAX_COLUMNS) return false;
                exc[n_exc++] = SamExc{(uint32_t)col, (uint32_t)SAMX_MIS << 24 | 1u, (uint32_t)(col - qi), c};
                ++j; ++col; ++qi; ++ref; --n;
                if (!sam_number(md, mn, j, left)) return false;
            }
        } else if (op == 'I') {
            if (stage > 3) return false;
            stage = 3;
            if (n) {
                if (col + n >= NS_SAM_MAX_COLUMNS) return false;
                exc[n_exc++] = SamExc{(uint32_t)col, (uint32_t)SAMX_INS << 24 | (uint32_t)n, (uint32_t)(col - qi), 0u};
                col += n; qi += n;
            }
        } else if (op == 'D') {
            if (stage > 3) return false;
            stage = 3;
            while (n) {
                if (!in_del) {
                    if (left || j + 1 >= mn || md[j] != '^' || !sam_is_letter(md[j + 1])) return false;   // a D column meets anything else
                    ++j; in_del = true;
                }
                uint64_t k = 0;
                while (k < n && j + k < mn && sam_is_letter(md[j + k])) ++k;
                if (col + k >= NS_SAM_MAX_COLUMNS) return false;
                exc[n_exc++] = SamExc{(uint32_t)col, (uint32_t)SAMX_DEL << 24 | (uint32_t)k, (uint32_t)(col - qi), (uint32_t)j};
                j += k; col += k; ref += k; n -= k;
                if (j >= mn || !sam_is_letter(md[j])) {                 // the run is over: its number follows
                    in_del = false;
                    if (!sam_number(md, mn, j, left)) return false;
                }
            }
        } else return false;
    }
    if (in_del || left || j < mn) return false;                          // MD has items left over
    if (head + tail + qi != sn || col >= NS_SAM_MAX_COLUMNS) return false;
    if (head > 0xffffffffull || tail > 0xffffffffull) return false;
    F.head = (uint32_t)head; F.tail = (uint32_t)tail; F.ref_len = (uint32_t)ref; F.query_len = (uint32_t)qi; F.cols = (uint32_t)col; F.n_exc = n_exc;
    return true;
}

// Where column c lies in a record's list: e = the first exception that ends behind c (n: none), past = the deleted columns in front of
// the end of exception e - 1 — what a column behind the last exception needs.
struct SamCursor { uint32_t e, past; SamExc cur; };
NS_CSH uint32_t sam_exc_past(const SamExc &x) { return x.ndel + (sam_exc_kind(x) == SAMX_DEL ? sam_exc_len(x) : 0u); }
NS_CSH void sam_cursor_at(SamCursor &k, const SamExc *x, uint32_t n, uint32_t c) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        const SamExc m = x[mid];
        if (m.col + sam_exc_len(m) > c) hi = mid; else lo = mid + 1u;
    }
    k.e = lo; k.past = 0; k.cur = SamExc{0u, 0u, 0u, 0u};
    if (lo > 0) k.past = sam_exc_past(x[lo - 1u]);
    if (lo < n) k.cur = x[lo];
}
// the two bytes of column c; the columns of a cursor are asked for in ascending order.  seq / md: the bytes of ALL records, seq_at /
// md_at: where this record's begin in them (plus its head clip for seq_at)
template <class S>
NS_CSH void sam_column(SamCursor &k, const SamExc *x, uint32_t n, uint32_t c, S &seq, uint64_t seq_at, S &md, uint64_t md_at, uint8_t &r, uint8_t &q) {
    while (k.e < n && k.cur.col + sam_exc_len(k.cur) <= c) { k.past = sam_exc_past(k.cur); ++k.e; if (k.e < n) k.cur = x[k.e]; }
    if (k.e < n && c >= k.cur.col) {
        const uint32_t kind = sam_exc_kind(k.cur);
        if (kind == SAMX_DEL) { r = md[md_at + k.cur.arg + (c - k.cur.col)]; q = '-'; return; }
        q = seq[seq_at + c - k.cur.ndel];
        r = kind == SAMX_INS ? (uint8_t)'-' : (uint8_t)k.cur.arg;
        return;
    }
    q = seq[seq_at + c - (k.e < n ? k.cur.ndel : k.past)];
    r = q;
}
