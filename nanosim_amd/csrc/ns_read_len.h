// ns_read_len.h — training side, the read-length models ("Read lengths: the KDE inputs"): what src/head_align_tail_dist.py
// (head_align_tail, A:58-281) takes from every primary alignment through pysam, restated from the CIGAR text alone, and the rule by
// which it joins the alignments of one read into aligned segments.  A: = src/head_align_tail_dist.py of bcgsc/NanoSim v3.2.2.
//
// Per record (len_scan_record, one record per thread in k_len_scan):
//   read_len      = infer_read_length()      = M + I + S + H + `=` + X
//   ref_len       = reference_length         = M + D + N + `=` + X
//   query_aln_len = query_alignment_length   = M + I + `=` + X
//   head, tail    = get_head_tail (A:38-55): the count of the FIRST op and of the LAST op when that op is S or H, else 0 — nothing but
//                   these two ops is looked at, so `5H10S…` gives 5 —, swapped when the record is reverse (FLAG 0x10)
//   edge          = edge_checker(start, start + ref_len, LN) (A:25-35): LEN_EDGE_START | LEN_EDGE_END.  The reference's `elif` is kept —
//                   an alignment that reaches the end is never also marked at the start — and nothing is marked when ref_len < 100.
// A record is BAD — all figures 0 — when its CIGAR is empty, holds a byte that is neither a digit nor one of MIDNSHP=X, has an op
// without a count (or a count without an op), has a sum beyond 32 bits, or has ref_len == 0 (the reference's `aligned_ref != 0`, A:172,
// silently drops the read such a record ends; here it is an error of the input).
//
// Per read (len_starts_segment): in genome mode a record goes on with the segment of the record in front of it when it is not the
// first record of its read, its reference is that of the PREVIOUS record (A:169 updates last_ref) and its edge is opposite to the edge
// of the read's FIRST record (A:156, 211: last_is_edge is never updated inside a read — kept).  Every other record, and every record in
// transcriptome mode, starts a segment.  A segment is the sum of its records' ref_len; a read has the largest read_len and the smallest
// head and tail of its records.
// The code below compiles for the device (k_len_scan, k_len_flag in ns_train.h) and, unchanged, for the host (tests/read_len_host.cpp).
#pragma once
#include <stdint.h>
#include "ns_sam_pairs.h"

enum { LEN_EDGE_START = 1, LEN_EDGE_END = 2 };
enum { LEN_GENOME = 0, LEN_TRANSCRIPTOME = 1 };
#define NS_LEN_EDGE_DIST 400u          // ref_edge_max_dist (A:25)
#define NS_LEN_EDGE_MIN_ALN 100u       // query_min_aln_len (A:25)
#define NS_LEN_NONE 0xffffffffu        // extra_head / extra_tail: the read is not in the genome alignments

struct LenFigures { uint32_t head, tail, read_len, ref_len, query_aln_len, edge; };

NS_CSH uint32_t len_edge(uint64_t start, uint64_t ref_len, uint64_t ref_total) {
    if (ref_len < NS_LEN_EDGE_MIN_ALN) return 0u;
    if (start + ref_len + 1u + NS_LEN_EDGE_DIST >= ref_total) return LEN_EDGE_END;       // rend >= LN - 1 - 400
    if (start <= NS_LEN_EDGE_DIST) return LEN_EDGE_START;
    return 0u;
}

// The walk over one record.  cg: its CIGAR bytes (cn of them); start: its 0-based reference start (POS - 1); ref_total: LN of its
// reference.  false: the record is bad (F is all zero then).
template <class S>
NS_CSH bool len_scan_record(S &cg, uint64_t cn, bool reverse, uint64_t start, uint64_t ref_total, LenFigures &F) {
    F.head = F.tail = F.read_len = F.ref_len = F.query_aln_len = F.edge = 0;
    if (!cn) return false;
    uint64_t both = 0, query_only = 0, ref_only = 0, clip = 0;      // M = X | I | D N | S H
    uint64_t first = 0, last = 0;                                    // the count of the first / last op when it is a clip, else 0
    bool is_first = true;
    uint64_t i = 0;
    while (i < cn) {
        uint64_t n;
        if (!sam_number(cg, cn, i, n) || i >= cn) return false;     // an op without a count, a byte that is no op, a count without an op
        const uint8_t op = cg[i++];
        last = 0;
        if (op == 'M' || op == '=' || op == 'X') both += n;
        else if (op == 'I') query_only += n;
        else if (op == 'D' || op == 'N') ref_only += n;
        else if (op == 'S' || op == 'H') { clip += n; last = n; }
        else if (op != 'P') return false;
        if (is_first) { first = last; is_first = false; }
        // (sam_number saturates at 2^40 and every sum is left as soon as it passes 2^32: no 64-bit sum can wrap)
        if (both + query_only + clip > 0xffffffffull || both + ref_only > 0xffffffffull) return false;
    }
    if (both + ref_only == 0) return false;
    F.head = (uint32_t)(reverse ? last : first); F.tail = (uint32_t)(reverse ? first : last);
    F.read_len = (uint32_t)(both + query_only + clip);
    F.ref_len = (uint32_t)(both + ref_only);
    F.query_aln_len = (uint32_t)(both + query_only);
    F.edge = len_edge(start, F.ref_len, ref_total);
    return true;
}

// does a record start an aligned segment?  first_in_read: it is the first record of its read; same_ref: its reference is the one of
// the record in front of it; first_edge: the edge of the read's first record; edge: its own
NS_CSH bool len_starts_segment(int mode, bool first_in_read, bool same_ref, uint32_t first_edge, uint32_t edge) {
    if (mode != LEN_GENOME || first_in_read || !same_ref) return true;
    const bool circular = ((first_edge & LEN_EDGE_START) && (edge & LEN_EDGE_END)) || ((first_edge & LEN_EDGE_END) && (edge & LEN_EDGE_START));
    return !circular;
}
