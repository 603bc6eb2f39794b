// ns_ir_train.h — training side, the intron-retention model ("Intron retention: the Markov counts"): what intron_retention of
// src/model_intron_retention.py (M:35-219) counts for every read that has a genome alignment and a transcriptome alignment — which
// introns of its transcript the read retains, and from that the six counts behind <prefix>_IR_markov_model.  M: =
// src/model_intron_retention.py of bcgsc/NanoSim v3.2.2.
//
// Per read (ir_walk_read, then ir_markov_read; one read per thread in k_ir_walk):
//   blocks    (pysam get_blocks, M:80) one block per M / = / X op of the CIGAR; D and N move the reference position, I / S / H / P do
//             not — an I between two M ops leaves two blocks that touch.  A block of 0 bases has no stretch.
//   stretches (M:119-132) every block is cut into stretches that lie inside or outside the union of the introns of the READ'S TRANSCRIPT
//             on the read's chromosome (the merged, sorted intervals the caller hands in: touching introns are one interval — the steps
//             HTSeq makes inside a stretch, from introns of other transcripts or from two introns that touch, change neither the sum nor
//             the smallest and largest end).  An inside stretch adds its length to the run (length_IR) and its two ends to the run's
//             positions; an outside stretch ends the run.
//   a run     is NOT ended by the end of a block: it goes on across D, N and I when the next block begins inside an intron (M:114 sets
//             length_IR once per read).  A run that is still open behind the last block is dropped (M:125 is only reached by an outside
//             stretch).
//   flush     (M:125-132) when a run ends, its length is compared with the length of EVERY intron of the transcript — by length alone:
//             a run over one half of each of two introns that is as long as a third one counts —; with an equal one the smallest and
//             the largest position of the run are recorded (once per equal intron there; a set here) and the read has ir_info.
//   retained  (M:147-176) intron i of the transcript, in file order, is retained by the read iff a recorded position p has
//             start_i <= p <= end_i — both ends inclusive, the chromosome not compared.  Here the two positions of a run are applied to
//             the introns when the run ends: a bit per intron in the read's row.
//   counts    (M:138-176) a read without ir_info whose transcript has introns: first[no_IR] += 1, states[no_IR][no_IR] += n - 1.  With
//             ir_info: first[state of intron 0] += 1, states[state of intron i - 1][state of intron i] += 1 for i = 1 .. n - 1.
// A read whose transcript has no intron (trx == NS_IR_NONE: absent from the annotation, or no intron row) counts nothing; a read on a
// chromosome without introns (chrom == NS_IR_NONE) has outside stretches only.
// A CIGAR is BAD — the read counts nothing — when it is empty, holds a byte that is neither a digit nor one of MIDNSHP=X, has an op
// without a count (or a count without an op), or moves the reference position beyond 2^32 - 1.
// The code below compiles for the device (k_ir_walk in ns_train.h) and, unchanged, for the host (tests/ir_train_host.cpp).
#pragma once
#include <stdint.h>
#include "ns_sam_pairs.h"

#define NS_IR_NONE_V 0xffffffffu                                       // NS_IR_NONE
enum { IR_READ_NONE = 0, IR_READ_NO_IR = 1, IR_READ_IR = 2 };          // the state byte of a read (NS_IR_READ_*)
enum { IRC_FIRST = 0, IRC_STATES = 2, IRC_WORDS = 6 };                 // first[2], states[2 * previous + current]

// the tables of a call (= ns_ir_introns): per transcript its introns in file order and the merged intervals
struct IrTables {
    uint32_t n_trx, n_chrom;
    const uint64_t *intr_off;
    const uint32_t *intr_chrom, *intr_start, *intr_end;
    const uint64_t *merged_off;
    const uint32_t *merged_chrom, *merged_start, *merged_end;
};
// one transcript of them
struct IrTrx {
    const uint32_t *start, *end; uint64_t n;                           // introns in file order
    const uint32_t *m_chrom, *m_start, *m_end; uint64_t m;             // merged intervals, sorted by (chromosome, start)
};
NS_CSH IrTrx ir_trx(const IrTables &T, uint32_t t) {
    if (t == NS_IR_NONE_V) return IrTrx{nullptr, nullptr, 0u, nullptr, nullptr, nullptr, 0u};
    const uint64_t a = T.intr_off[t], b = T.merged_off[t];
    return IrTrx{T.intr_start + a, T.intr_end + a, T.intr_off[t + 1] - a, T.merged_chrom + b, T.merged_start + b, T.merged_end + b, T.merged_off[t + 1] - b};
}
NS_CSH uint64_t ir_row_words(uint64_t n_introns) { return (n_introns + 31u) >> 5; }

// what a call refuses: nullptr when the tables and the reads' ids are in order, else what is wrong
NS_CSH const char *ir_check_tables(const IrTables &T) {
    if (!T.intr_off || !T.merged_off) return "null argument";
    if (T.intr_off[0] != 0 || T.merged_off[0] != 0) return "intr_off / merged_off does not begin at 0";
    for (uint32_t t = 0; t < T.n_trx; ++t)
        if (T.intr_off[t] > T.intr_off[t + 1] || T.merged_off[t] > T.merged_off[t + 1]) return "intr_off / merged_off decreases";
    const uint64_t ni = T.intr_off[T.n_trx], nm = T.merged_off[T.n_trx];
    if (ni >= (1ull << 31) || nm >= (1ull << 31)) return "2^31 introns or more";
    if ((ni && (!T.intr_chrom || !T.intr_start || !T.intr_end)) || (nm && (!T.merged_chrom || !T.merged_start || !T.merged_end))) return "null argument";
    for (uint64_t i = 0; i < ni; ++i) {
        if (T.intr_chrom[i] >= T.n_chrom) return "chromosome id of an intron is not below n_chrom";
        if (T.intr_end[i] < T.intr_start[i]) return "an intron ends in front of its start";
    }
    for (uint32_t t = 0; t < T.n_trx; ++t)
        for (uint64_t k = T.merged_off[t]; k < T.merged_off[t + 1]; ++k) {
            if (T.merged_chrom[k] >= T.n_chrom) return "chromosome id of a merged interval is not below n_chrom";
            if (T.merged_end[k] <= T.merged_start[k]) return "a merged interval is empty";
            if (k > T.merged_off[t] && (T.merged_chrom[k] < T.merged_chrom[k - 1] ||
                                        (T.merged_chrom[k] == T.merged_chrom[k - 1] && T.merged_start[k] <= T.merged_end[k - 1])))
                return "merged intervals are not sorted, or two of them overlap or touch";
        }
    return nullptr;
}
NS_CSH const char *ir_check_reads(const IrTables &T, const uint32_t *chrom, const uint32_t *trx, uint32_t n_reads) {
    for (uint32_t r = 0; r < n_reads; ++r) {
        if (chrom[r] != NS_IR_NONE_V && chrom[r] >= T.n_chrom) return "chromosome id of a read is neither below n_chrom nor NS_IR_NONE";
        if (trx[r] != NS_IR_NONE_V && trx[r] >= T.n_trx) return "transcript id of a read is neither below n_trx nor NS_IR_NONE";
    }
    return nullptr;
}

// the first merged interval at or behind k that ends behind `pos` on `chrom`, or lies on a later chromosome (X.m without)
NS_CSH uint64_t ir_locate(const IrTrx &X, uint64_t k, uint32_t chrom, uint64_t pos) {
    uint64_t lo = k, hi = X.m;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        const uint32_t c = X.m_chrom[mid];
        if (c < chrom || (c == chrom && (uint64_t)X.m_end[mid] <= pos)) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// a run ends (M:125-132): row gets the introns that one of its two positions lies in, when an intron is as long as the run
NS_CSH void ir_flush(const IrTrx &X, uint64_t length_ir, uint32_t mn, uint32_t mx, uint32_t *row, bool &ir_info) {
    bool equal = false;
    for (uint64_t i = 0; i < X.n && !equal; ++i) equal = (uint64_t)(X.end[i] - X.start[i]) == length_ir;
    if (!equal) return;
    ir_info = true;
    for (uint64_t i = 0; i < X.n; ++i) {
        const uint32_t s = X.start[i], e = X.end[i];
        if ((s <= mn && mn <= e) || (s <= mx && mx <= e)) row[i >> 5] |= 1u << (i & 31u);
    }
}

// The walk over one read.  cg: its CIGAR bytes (cn of them); start: its 0-based reference start; chrom: its chromosome id or NS_IR_NONE;
// X: its transcript (ir_trx); row: ir_row_words(X.n) words, zeroed by the caller.  false: the CIGAR is bad (row is undefined then).
template <class S>
NS_CSH bool ir_walk_read(S &cg, uint64_t cn, uint32_t start, uint32_t chrom, const IrTrx &X, uint32_t *row, bool &ir_info) {
    ir_info = false;
    if (!cn) return false;
    uint64_t pos = start, length_ir = 0, k = 0;
    uint32_t mn = 0xffffffffu, mx = 0u;
    uint64_t i = 0;
    while (i < cn) {
        uint64_t n;
        if (!sam_number(cg, cn, i, n) || i >= cn) return false;     // an op without a count, a byte that is no op, a count without an op
        const uint8_t op = cg[i++];
        if (op == 'I' || op == 'S' || op == 'H' || op == 'P') continue;
        if (op != 'M' && op != '=' && op != 'X' && op != 'D' && op != 'N') return false;
        const uint64_t end = pos + n;                                 // (sam_number saturates at 2^40: no wrap)
        if (end > 0xffffffffull) return false;
        if (op == 'M' || op == '=' || op == 'X') {
            while (pos < end) {
                k = ir_locate(X, k, chrom, pos);
                const bool here = k < X.m && X.m_chrom[k] == chrom;
                if (here && (uint64_t)X.m_start[k] <= pos) {          // inside, up to the interval's end or the block's
                    const uint64_t e = (uint64_t)X.m_end[k] < end ? (uint64_t)X.m_end[k] : end;
                    length_ir += e - pos;
                    if ((uint32_t)pos < mn) mn = (uint32_t)pos;
                    if ((uint32_t)e > mx) mx = (uint32_t)e;
                    pos = e;
                } else {                                              // outside, up to the next interval or the block's end
                    if (length_ir) { ir_flush(X, length_ir, mn, mx, row, ir_info); length_ir = 0; mn = 0xffffffffu; mx = 0u; }
                    pos = here && (uint64_t)X.m_start[k] < end ? (uint64_t)X.m_start[k] : end;
                }
            }
        }
        pos = end;
    }
    return true;
}

// The six counts of one read (M:138-176) from its row.  n: the introns of its transcript; c[IRC_WORDS] is added to.  -> IR_READ_*
NS_CSH uint32_t ir_markov_read(uint64_t n, const uint32_t *row, bool ir_info, unsigned long long *c) {
    if (!n) return IR_READ_NONE;
    if (!ir_info) { c[IRC_FIRST] += 1u; c[IRC_STATES] += n - 1u; return IR_READ_NO_IR; }
    uint32_t prev = row[0] & 1u;
    c[IRC_FIRST + prev] += 1u;
    for (uint64_t i = 1; i < n; ++i) {
        const uint32_t cur = (row[i >> 5] >> (i & 31u)) & 1u;
        c[IRC_STATES + 2u * prev + cur] += 1u;
        prev = cur;
    }
    return IR_READ_IR;
}
