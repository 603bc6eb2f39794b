// ns_hp_hist.h — training side, the homopolymer-length model: what src/model_homopolymer_lengths.py collects from the two
// aligned lines of every MAF alignment — per homopolymer of the reference its length there and the length the read shows for it
// (analyze_homopolymers, H:64-119), and the column counts behind the homopolymer mismatch rate (calc_homopolymer_mis_rate, H:9-33) —
// as ONE left-to-right pass per alignment.  H: = src/model_homopolymer_lengths.py of bcgsc/NanoSim v3.2.2.
//
// The reference runs four regular expressions per alignment.  Restated (k = min_hp_len >= 1):
//  * `A{k,}|C{k,}|G{k,}|T{k,}` over the dash-less reference line (H:64-68): a homopolymer is a maximal run of one of the four upper-case
//    letters with at least k letters; lower case, N and every other byte end a run and never form one.
//  * `(-*A-*){k,}|...` over the reference line (H:70-73), zipped with the former: the homopolymer's aligned span.  It begins at the first
//    '-' of the dash run directly in front of the first letter — unless a homopolymer ended in front of those dashes: a match takes its
//    trailing dashes — and ends behind the dashes that follow the last letter.  A run that is too short matches nothing, so the dashes
//    behind it stay available to the next run.
//  * `(BB+){s<=1}` over the read's bytes of the span without '-' (H:86-106), B the homopolymer's base: a greedy scan — from position p
//    the stretch grows while the byte is B or is the FIRST byte that is not B; a stretch of two or more bytes is a match and the scan
//    goes on behind it, otherwise at p + 1 (in both cases at the second byte that is not B).  A match counts its length without a first
//    and without a last byte that is not B; read_len is the largest count, 0 without a match.
//  * calc_homopolymer_mis_rate over the spans: '-' in the reference part are insertions, '-' in the read part deletions, a column
//    without '-' is a match (equal bytes, case-sensitive) or a mismatch.
// A run is known to be a homopolymer only at its k-th letter and to have ended only at the next other letter, so the walk gathers a
// span's figures while the run lasts (HpSpan) and hands them on or drops them when it ends.  The dashes in front of a run are met
// before its base is known: the walk remembers where they begin and feeds those few columns to the new span when the run starts.
// The code below compiles for the device (k_hp_count, k_hp_records) and, unchanged, for the host (tests/hp_train_host.cpp).
#pragma once
#include <stdint.h>
#include "ns_cs_hist.h"

enum { HPH_AT = 0, HPH_CG = 1 };                               // the two rows of the reference's file (H:116)
enum { HPC_INS = 0, HPC_DEL = 1, HPC_MIS = 2, HPC_MATCH = 3 }; // err_dict (H:15)

// what the span of the current run has gathered
struct HpSpan {
    uint32_t ref_len;                  // letters of the reference
    uint32_t col[4];                   // HPC_*
    uint32_t len, best;                // the fuzzy scan: bytes of the stretch that is open, the best count of those that are closed
    bool used, first_bad, last_bad;    // the stretch holds a byte that is not the base; its first / its last byte is one
};
NS_CSH void hp_span_init(HpSpan &s) {
    s.ref_len = 0; s.col[0] = s.col[1] = s.col[2] = s.col[3] = 0; s.len = s.best = 0; s.used = s.first_bad = s.last_bad = false;
}
NS_CSH void hp_scan_close(HpSpan &s) {
    if (s.len >= 2u) { const uint32_t v = s.len - (s.first_bad ? 1u : 0u) - (s.last_bad ? 1u : 0u); s.best = s.best > v ? s.best : v; }
}
// the next byte of the read segment
NS_CSH void hp_scan_byte(HpSpan &s, bool bad) {
    if (!s.len) { s.len = 1; s.used = s.first_bad = s.last_bad = bad; }
    else if (!bad) { ++s.len; s.last_bad = false; }
    else if (!s.used) { ++s.len; s.used = s.last_bad = true; }
    else { hp_scan_close(s); s.len = 1; s.used = s.first_bad = s.last_bad = true; }     // the second one: the next stretch begins with it
}
// one column of the span: r, q = the bytes of the two lines
NS_CSH void hp_span_column(HpSpan &s, uint8_t base, uint8_t r, uint8_t q) {
    if (r == '-') ++s.col[HPC_INS]; else ++s.ref_len;
    if (q == '-') { ++s.col[HPC_DEL]; return; }
    hp_scan_byte(s, q != base);
    if (r != '-') ++s.col[r == q ? HPC_MATCH : HPC_MIS];
}
NS_CSH uint32_t hp_read_len(HpSpan &s) { hp_scan_close(s); s.len = 0; return s.best; }

// read_len of a dash-less read segment alone (the CPU tests compare it with the `regex` module)
template <class S>
NS_CSH uint32_t hp_fuzzy_len(S &seg, uint64_t n, uint8_t base) {
    HpSpan s; hp_span_init(s);
    for (uint64_t i = 0; i < n; ++i) hp_scan_byte(s, seg[i] != base);
    return hp_read_len(s);
}

// The walk over one alignment.  Per homopolymer acc.hp(class, base, ref_len, read_len, start, end) — start / end: its letters in the
// dash-less reference line, [start, end) —, then once acc.columns(ins, del, mis, match) summed over its spans.  Returns the number of
// homopolymers.  Lines of up to 2^32 - 1 columns (the callers refuse longer ones).
template <class Acc, class S>
NS_CSH uint32_t hp_hist_alignment(S &ref, S &qry, uint64_t n, uint32_t k, Acc &acc) {
    HpSpan sp; hp_span_init(sp);
    uint32_t col[4] = {0u, 0u, 0u, 0u}, n_hp = 0;
    uint8_t base = 0;                          // the letter of the run that is open (0: none)
    uint32_t letters = 0, run_start = 0;       // letters of the reference met so far; where the open run begins among them
    uint64_t dash_from = 0; bool dashes = false;   // the dash run that ends in front of column i and that no homopolymer has taken
    auto close_run = [&]() -> bool {           // true: it was a homopolymer (and took the dashes behind it)
        if (!base || sp.ref_len < k) return false;
        acc.hp((base == 'A' || base == 'T') ? (uint32_t)HPH_AT : (uint32_t)HPH_CG, base, sp.ref_len, hp_read_len(sp), run_start, run_start + sp.ref_len);
        for (int c = 0; c < 4; ++c) col[c] += sp.col[c];
        ++n_hp;
        return true;
    };
    for (uint64_t i = 0; i < n; ++i) {
        const uint8_t r = ref[i];
        if (r == '-') {
            if (!dashes) { dashes = true; dash_from = i; }
            if (base) hp_span_column(sp, base, r, qry[i]);          // behind the run's letters: its own if it goes on or is long enough
            continue;
        }
        if (r != base) {                                            // another letter: the open run is over
            const bool took = close_run();
            base = (r == 'A' || r == 'C' || r == 'G' || r == 'T') ? r : (uint8_t)0;
            if (base) {
                hp_span_init(sp); run_start = letters;
                if (dashes && !took) for (uint64_t j = dash_from; j < i; ++j) hp_span_column(sp, base, '-', qry[j]);
            }
        }
        if (base) hp_span_column(sp, base, r, qry[i]);
        ++letters; dashes = false;
    }
    close_run();
    acc.columns(col[HPC_INS], col[HPC_DEL], col[HPC_MIS], col[HPC_MATCH]);
    return n_hp;
}
