// ns_qual_hist.h — training side, the base-quality model: what src/model_base_qualities.py collects per query base of
// every primary alignment (M:23-79) — the base's class (mismatch / insertion / match / head-tail clip / unmapped read) and its quality —
// as a 5 x 94 histogram; the log-normal fit of M:82-96 is a closed form of that histogram (nanosim_amd/characterize/qualities.py).
// M: = src/model_base_qualities.py of bcgsc/NanoSim v3.2.2.
//
// Two phases.  MARK: one walk per alignment over its cs string (the tokeniser of ns_cs_hist.h, cs_next_item — the regex of M:25 is the
// one of parse_cs) with a cursor on the query; only the EXCEPTIONS are recorded, one 2-bit mark per mismatched and per inserted base,
// in a zero-initialised side array over the quality bytes (16 bases per 32-bit word).  COUNT: the quality bytes and the marks are
// streamed once, whatever the alignment boundaries; clips and unmapped reads are decided by position (qual_class), not marked.
// The code below compiles for the device (k_qual_mark, k_qual_count) and, unchanged, for the host (tests/qual_hist_host.cpp).
#pragma once
#include <stdint.h>
#include "ns_cs_hist.h"

enum { QH_MIS = 0, QH_INS = 1, QH_MATCH = 2, QH_HT = 3, QH_UNMAPPED = 4, QH_CLASSES = 5 };   // the order of fit_lognorm's rows (M:62, 85)
enum { QM_NONE = 0, QM_MIS = 1, QM_INS = 2 };                                                 // a base's mark
#define NS_QUAL_FIRST 33u         // '!': Phred + 33
#define NS_QUAL_VALUES 94u        // '!' .. '~'

// The walk of convert_cs + the loop of analyze_aligned_base_qualities (M:23-36, 69-75) over one alignment: `aligned` = the length of
// query_alignment_sequence (QUAL without the soft clips); sink.mark(i, QM_*) for base i of the aligned part, in ascending i.  The walk
// stops at the aligned length (cs_arr entries behind it are never looked at); false: the string covers fewer bases (the reference stops
// with an IndexError there).  `-seq` and `=seq` items contribute nothing (M:33-34).
template <class Sink, class S>
NS_CSH bool qual_mark_alignment(S &s, uint64_t n, uint64_t aligned, Sink &sink) {
    uint64_t i = 0, q = 0;
    int t; uint32_t l;
    while (q < aligned && cs_next_item(s, n, i, t, l)) {
        if (t == CS_MATCH) q += l;
        else if (t == CS_MIS) { sink.mark(q, QM_MIS); ++q; }
        else if (t == CS_INS) {
            const uint64_t e = q + l < aligned ? q + l : aligned;
            for (uint64_t k = q; k < e; ++k) sink.mark(k, QM_INS);
            q += l;
        }
    }
    return q >= aligned;
}

// the class of base `rel` of an alignment whose quality string has `len` bytes (M:39-52, 73-75; P:172-175 for unmapped reads)
NS_CSH uint32_t qual_class(uint64_t rel, uint64_t len, uint32_t head, uint32_t tail, uint32_t unmapped, uint32_t mark) {
    if (unmapped) return QH_UNMAPPED;
    if (rel < head || rel >= len - tail) return QH_HT;
    return mark == QM_MIS ? QH_MIS : mark == QM_INS ? QH_INS : QH_MATCH;
}

// the alignment that holds byte `pos` of the quality strings: the smallest a in [lo, n_aln) with off[a + 1] > pos (empty strings hold
// nothing); n_aln when there is none
NS_CSH uint32_t qual_locate(const uint64_t *off, uint32_t lo, uint32_t n_aln, uint64_t pos) {
    uint32_t hi = n_aln;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (off[mid + 1] > pos) hi = mid; else lo = mid + 1u;
    }
    return lo;
}
