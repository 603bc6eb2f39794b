// ns_maf_best.h — training side, the best hit per read of LAST's MAF alignments ("MAF input: the best hit per read"): what
// besthit_and_unaligned of src/get_besthit_maf.py (G:8-56) keeps of the `s` lines of a MAF file.  G: = src/get_besthit_maf.py of
// bcgsc/NanoSim v3.2.2.
//
// The `s` lines come in pairs (reference line, then query line).  Of the pairs of one query name the reference keeps the one with the
// largest `size` (field 3 of the query line; G:14-22 replaces only on strictly greater), and of several with that size the first in the
// file (G:34: the first pair that equals the maximum marks the name done).  The kept pairs are written in file order, both lines verbatim.
//   lines   (maf_is_start) a byte starts an `s` line when it is the first of the file or follows '\n', is 's', and a space or a tab follows
//           it — the filter of characterize.maf_pairs: `#` headers, `a score=` lines and blank lines are no lines here.  A line ends in
//           front of the next '\n' or at the end of the text.
//   fields  (maf_parse_line) Python's split(): runs of space, \t, \r, \v, \f separate.  Field 1 the name, 2 `start`, 3 `size`, 4 the strand,
//           5 `srcSize`, 6 the aligned sequence; 2, 3 and 5 are plain decimal digits that fit 32 bits.  Anything else — a sign, an
//           underscore, an overflow, fewer than 7 fields — makes the line BAD (Python's int() takes more; LAST writes digits).
//   choice  (maf_claim, maf_offer) an open-addressing table with linear probing, one 32-bit owner word (a pair index, MAF_EMPTY without)
//           and one 64-bit key word per slot.  A pair finds the slot of its query name by compare-and-swap on the owner words — it looks at
//           a slot ONLY through the value the compare-and-swap returns — and compares the bytes of its name with the owner's name in the
//           text, which nobody writes: the hash only says where to begin.  The walk is bounded by the table's size.  Then one 64-bit
//           maximum of (size << 32) | (0xffffffff - pair) on the key word: the largest size, and of equal sizes the smallest pair index,
//           whatever the order in which the pairs arrive.  Nothing waits for another pair.
//   result  (maf_kept, after every pair has offered) a pair is kept iff the key of its slot names it.  pos_strand counts the kept pairs whose
//           two strand fields are equal as byte strings (G:38).
//   names   (maf_find) the names of a reads file are looked up in the settled table: found = it was a QUERY name (G:48).
// The code below compiles for the device (k_maf_* in ns_train.h) and, unchanged, for the host (tests/maf_best_host.cpp), where the two
// table operations are plain reads and writes (the `Ops` argument).
#pragma once
#include <stdint.h>
#include "ns_cs_hist.h"

#define MAF_EMPTY 0xffffffffu
#define MAF_LINE_SPAN 16384u                          // the bytes of the text one workgroup of the line kernels looks at (256 threads x 64)
#define MAF_LINE_PER_THREAD 64u

// one `s` line: where its fields stand in the text (begin offsets; the line's own begin is the caller's)
struct MafLine {
    uint64_t end;                                     // one past its last byte: the '\n' or the end of the text
    uint64_t name_at, strand_at, seq_at;
    uint32_t name_len, strand_len, seq_len;
    uint32_t start, size, src_size;
};

NS_CSH bool maf_is_space(uint8_t c) { return c == ' ' || (c >= 9u && c <= 13u && c != '\n'); }          // split()'s separators inside a line
template <class S> NS_CSH bool maf_is_start(S &t, uint64_t nbytes, uint64_t i) {
    if (i + 1u >= nbytes || t[i] != 's') return false;
    const uint8_t c = t[i + 1u];
    return (c == ' ' || c == '\t') && (i == 0 || t[i - 1u] == '\n');
}

// the line that begins at `at`; false: a bad line (L is then not to be used beyond `end`, which is always set)
template <class S> NS_CSH bool maf_parse_line(S &t, uint64_t nbytes, uint64_t at, MafLine &L) {
    uint64_t i = at + 1u;                             // (behind the `s`)
    uint32_t field = 1;
    bool ok = true;
    L.name_at = L.strand_at = L.seq_at = 0; L.name_len = L.strand_len = L.seq_len = 0; L.start = L.size = L.src_size = 0;
    for (;;) {
        uint8_t c = 0;
        while (i < nbytes && maf_is_space(c = t[i])) ++i;
        if (i >= nbytes || c == '\n') break;
        const uint64_t b = i;
        uint64_t v = 0;
        bool digits = true;
        const bool number = field == 2u || field == 3u || field == 5u;
        while (i < nbytes && (c = t[i]) != '\n' && !maf_is_space(c)) {
            if (number) {
                if (c < '0' || c > '9') digits = false;
                else if (v <= 0xffffffffull) v = v * 10u + (c - '0');
            }
            ++i;
        }
        const uint64_t n = i - b;
        if (number && (!digits || v > 0xffffffffull)) ok = false;
        if (n > 0xffffffffull) ok = false;                         // (a span is 32 bits long)
        if (field == 1u) { L.name_at = b; L.name_len = (uint32_t)n; }
        else if (field == 2u) L.start = (uint32_t)v;
        else if (field == 3u) L.size = (uint32_t)v;
        else if (field == 4u) { L.strand_at = b; L.strand_len = (uint32_t)n; }
        else if (field == 5u) L.src_size = (uint32_t)v;
        else if (field == 6u) { L.seq_at = b; L.seq_len = (uint32_t)n; }
        if (field < 7u) ++field;
    }
    L.end = i;
    return ok && field == 7u;
}

template <class S> NS_CSH uint32_t maf_hash(S &t, uint64_t at, uint32_t n) {             // FNV-1a over the name, then a finaliser: where the walk begins
    uint32_t h = 2166136261u;
    for (uint32_t k = 0; k < n; ++k) h = (h ^ t[at + k]) * 16777619u;
    h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13;
    return h;
}
template <class S, class U> NS_CSH bool maf_same_bytes(S &a, uint64_t a_at, uint32_t a_len, U &b, uint64_t b_at, uint32_t b_len) {
    if (a_len != b_len) return false;
    for (uint32_t k = 0; k < a_len; ++k) if (a[a_at + k] != b[b_at + k]) return false;
    return true;
}

// the table: `slots` a power of two (>= 2 x pairs), owner[] preset to MAF_EMPTY, key[] to 0 (smaller than any offered key)
struct MafTable { uint32_t *owner; unsigned long long *key; uint64_t slots; };
NS_CSH unsigned long long maf_key(uint32_t size, uint32_t pair) { return (unsigned long long)size << 32 | (0xffffffffu - pair); }
NS_CSH uint32_t maf_key_pair(unsigned long long key) { return 0xffffffffu - (uint32_t)key; }

// pair p (its query line Q) finds or founds the slot of its name; `lines` = the parsed lines of the call (the query line of pair o is
// lines[2 o + 1]).  -> the slot, or T.slots when the table is exhausted (it never is at the size the callers give it).
// Ops::cas(word, expected, desired) -> the old value: the only look at an owner word.  t and u read the same text (two windows on the device).
template <class S, class Ops> NS_CSH uint64_t maf_claim(S &t, S &u, const MafLine *lines, const MafTable &T, uint32_t p, const MafLine &Q, Ops &ops) {
    uint64_t slot = maf_hash(t, Q.name_at, Q.name_len) & (T.slots - 1u);
    for (uint64_t tries = 0; tries < T.slots; ++tries) {
        const uint32_t o = ops.cas(T.owner + slot, MAF_EMPTY, p);
        if (o == MAF_EMPTY || o == p) return slot;
        const MafLine &O = lines[2ull * o + 1u];
        if (maf_same_bytes(t, Q.name_at, Q.name_len, u, O.name_at, O.name_len)) return slot;
        slot = (slot + 1u) & (T.slots - 1u);
    }
    return T.slots;
}
// Ops::max64(word, value): word = max(word, value) in one operation
template <class Ops> NS_CSH void maf_offer(const MafTable &T, uint64_t slot, uint32_t p, uint32_t size, Ops &ops) { ops.max64(T.key + slot, maf_key(size, p)); }
// after every pair has offered (on the device: in a later kernel)
NS_CSH bool maf_kept(const MafTable &T, uint64_t slot, uint32_t p) { return maf_key_pair(T.key[slot]) == p; }

// a name of the reads file (bytes `names`, from n_at, n_len long) in the settled table: was it a query name?
template <class S, class U> NS_CSH bool maf_find(S &t, const MafLine *lines, const MafTable &T, U &names, uint64_t n_at, uint32_t n_len) {
    uint64_t slot = maf_hash(names, n_at, n_len) & (T.slots - 1u);
    for (uint64_t tries = 0; tries < T.slots; ++tries) {
        const uint32_t o = T.owner[slot];
        if (o == MAF_EMPTY) return false;
        const MafLine &O = lines[2ull * o + 1u];
        if (maf_same_bytes(names, n_at, n_len, t, O.name_at, O.name_len)) return true;
        slot = (slot + 1u) & (T.slots - 1u);
    }
    return false;
}

// what a kept pair leaves (= ns_maf_best_lines, ns_maf_best_record, ns_maf_best_figures of include/nanosim_amd.h)
struct MafOutLines { uint64_t ref_begin, ref_end, qry_begin, qry_end; };                  // the two lines with their '\n' (where they have one)
struct MafOutRecord { uint64_t ref_name_at, ref_seq_at, qry_seq_at; uint32_t ref_name_len, ref_seq_len, qry_seq_len, ref_start; };
struct MafOutFigures { uint32_t aligned_ref, ref_total, head, total; int64_t ht; };     // A:91-110: r[3], r[5], q[2], q[5], q[5] - q[3]
NS_CSH void maf_emit(uint64_t nbytes, uint64_t r_at, const MafLine &R, uint64_t q_at, const MafLine &Q, MafOutLines &ol, MafOutRecord &orc, MafOutFigures &of) {
    ol = MafOutLines{r_at, R.end + (R.end < nbytes ? 1u : 0u), q_at, Q.end + (Q.end < nbytes ? 1u : 0u)};
    orc = MafOutRecord{R.name_at, R.seq_at, Q.seq_at, R.name_len, R.seq_len, Q.seq_len, R.start};
    of = MafOutFigures{R.size, R.src_size, Q.start, Q.src_size, (int64_t)Q.src_size - (int64_t)Q.size};
}
