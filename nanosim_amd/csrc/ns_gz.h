// ns_gz.h — compressed output ("BGZF output"): the record and error-profile images leave the device as BGZF members, a series
// of independent gzip members that `zcat`, Python's gzip, bgzip and htslib read.  A member holds at most NS_GZ_BLOCK_BYTES input bytes as ONE
// deflate block of literals only: a dynamic-Huffman block under a code that serves the whole stream (ns_gz_code, include/nanosim_amd.h),
// or a stored block when that is smaller or when the code lacks a byte of the block.  No LZ77 matching.
//
// Three parts:
//   the code     (host only: gz_code_build) a length-limited canonical Huffman code from a histogram, and the complete header of the
//                dynamic block as a bit string, which the block walk only copies;
//   the walk     (gz_member_size, gz_member: written against an abstract wavefront W like ns_calmd.h and ns_bam.h, so that it runs on 64
//                host threads in lock step under the sanitizers) ONE WAVEFRONT makes ONE member;
//   the kernels  (k_gz_hist, k_gz_size, k_gz_emit, k_gz_offsets: gfx950) sizes first, a device scan, then every member at its final place.
//
// THE WALK.  The block lies RIGHT-ALIGNED in a grid of 64 spans of GZ_SPAN bytes, one per lane: the last lane is always full, the lanes in
// front of the block are empty, and only the first lane with bytes is short.  So every lane behind the first one carries GZ_SPAN bytes —
// at least GZ_SPAN bits, more than a word — and its distance to the end of the block is fixed.
//   bits   each lane sums the code lengths of its span and notes a byte without a code; a prefix sum gives where its bits begin.
//   words  the member is built in a staging image of 32-bit words (LDS on the device) and EVERY WORD IS STORED BY EXACTLY ONE LANE:
//          the whole words of the prefix (the 18 bytes of the BGZF header and the block header's bits) by lane w for word w; the rest of
//          the prefix is what the first lane with bytes starts its accumulator with.  A lane owns the words whose first bit is its own;
//          the bits in front of its first word boundary — the tail of the word the lane before it began — travel to that lane by a
//          shuffle, which ORs them into its last word.  The last lane appends end-of-block, the padding and the trailer (CRC32, ISIZE).
//          A stored block takes the same path: its bytes are 8-bit codes, its header (BFINAL/BTYPE, LEN, NLEN) a bit string of 40 bits.
//   crc    each lane runs the table CRC over its span, the first lane with bytes from 0xffffffff and every other from 0; lane l's
//          register is multiplied by x^(8 * GZ_SPAN * (63 - l)) modulo the CRC polynomial — a constant per lane, because the grid is
//          right-aligned — and the products are XORed over the wavefront.
//   out    behind a fence the lanes copy the staging image to its place: aligned 32-bit stores, single bytes in front and behind.
#pragma once
#include <stdint.h>
#include <string.h>
#include "../../include/nanosim_amd.h"
#include "ns_cs_hist.h"

#define GZ_LANES 64u
#define GZ_SPAN (NS_GZ_BLOCK_BYTES / GZ_LANES)               // bytes per lane
#define GZ_STAGE_WORDS (NS_GZ_BLOCK_BYTES / 4u + 8u)         // the largest member: 18 + 5 + NS_GZ_BLOCK_BYTES + 8 bytes
#define GZ_HEADER_WORDS (NS_GZ_HEADER_BYTES / 4u)
#define GZ_HEADER_BITS_MAX 1880u                              // (include/nanosim_amd.h derives it)
#define GZ_BGZF_BITS 144u                                     // the 18 bytes in front of the deflate block
#define GZ_MEMBER_EXTRA 26u                                   // ... and the 8 behind it
#define GZ_STORED_EXTRA 5u                                    // BFINAL/BTYPE, LEN, NLEN
#define GZ_EOB 256u
#define GZ_CRC_POLY 0xedb88320u
static_assert(NS_GZ_BLOCK_BYTES % 64u == 0 && (NS_GZ_BLOCK_BYTES & (NS_GZ_BLOCK_BYTES - 1u)) == 0 && NS_GZ_BLOCK_BYTES <= 65280u, "a power-of-two multiple of 64 that BSIZE can hold");
static_assert((GZ_BGZF_BITS + GZ_HEADER_BITS_MAX) / 32u < GZ_LANES, "one lane per whole word of the prefix");
static_assert(GZ_SPAN >= 4u, "a full lane carries a word of bits or more");
static_assert(GZ_HEADER_BITS_MAX <= 8u * NS_GZ_HEADER_BYTES, "the header fits its array");

// what the walk reads of a code: sym[v] = len << 16 | code (v = 256: end-of-block), the header in words, and the two CRC tables
struct GzDevCode {
    uint32_t sym[257], header_bits;
    uint32_t header[GZ_HEADER_WORDS];
    uint32_t lane_pow[GZ_LANES];      // x^(8 * GZ_SPAN * (63 - l)) mod P, reflected like the CRC register (bit 31: x^0)
    uint32_t crc_tab[256];
};
struct GzTabs { const uint32_t *sym, *crc_tab, *header, *lane_pow; uint32_t header_bits; };

// ---------------------------------------------------------------------------------------------------------
// the code (host only)
// ---------------------------------------------------------------------------------------------------------
// lengths of a Huffman code over the n symbols with freq > 0, none longer than max_len (n <= 257).  The tree is built with two queues
// over the sorted leaves; lengths beyond max_len are cut and the Kraft sum is brought back to 1 by lengthening the shortest-lived codes
// one step at a time; the lengths go to the symbols by ascending frequency, longest first.  One symbol alone gets length 1.
static inline void gz_huff_lengths(const uint64_t *freq, uint32_t n_sym, uint32_t max_len, uint8_t *len) {
    uint32_t order[257], m = 0;
    for (uint32_t s = 0; s < n_sym; ++s) { len[s] = 0; if (freq[s]) order[m++] = s; }
    if (!m) return;
    if (m == 1) { len[order[0]] = 1; return; }
    for (uint32_t i = 1; i < m; ++i) {                               // insertion sort by (freq, symbol), ascending
        const uint32_t s = order[i]; uint32_t j = i;
        while (j && freq[order[j - 1]] > freq[s]) { order[j] = order[j - 1]; --j; }
        order[j] = s;
    }
    uint64_t wt[2 * 257]; uint32_t parent[2 * 257], depth[2 * 257];
    for (uint32_t i = 0; i < m; ++i) wt[i] = freq[order[i]];
    uint32_t leaf = 0, node = m, made = m;                           // next unused leaf, next unused inner node, nodes so far
    auto take = [&]() -> uint32_t { return (leaf < m && (node >= made || wt[leaf] <= wt[node])) ? leaf++ : node++; };
    while (made < 2 * m - 1) {
        const uint32_t a = take(), b = take();
        const uint64_t sum = wt[a] + wt[b];
        wt[made] = sum < wt[a] ? ~0ull : sum;                        // (saturates: counts near 2^64 still give a valid code)
        parent[a] = parent[b] = made++;
    }
    depth[made - 1] = 0;
    for (uint32_t i = made - 1; i-- > 0;) depth[i] = depth[parent[i]] + 1u;
    uint32_t num[33] = {0};
    for (uint32_t i = 0; i < m; ++i) num[depth[i] < max_len ? depth[i] : max_len]++;
    uint64_t total = 0;
    for (uint32_t l = 1; l <= max_len; ++l) total += (uint64_t)num[l] << (max_len - l);
    while (total > (1ull << max_len)) {
        num[max_len]--;
        for (uint32_t l = max_len - 1; l > 0; --l) if (num[l]) { num[l]--; num[l + 1] += 2; break; }
        total--;
    }
    uint32_t i = 0;
    for (uint32_t l = max_len; l > 0; --l) for (uint32_t k = 0; k < num[l]; ++k) len[order[i++]] = (uint8_t)l;
}
// the canonical codes of the lengths (RFC 1951 3.2.2), bit-reversed
static inline void gz_canonical(const uint8_t *len, uint32_t n_sym, uint32_t max_len, uint16_t *code) {
    uint32_t count[17] = {0}, next[17] = {0};
    for (uint32_t s = 0; s < n_sym; ++s) count[len[s]]++;
    count[0] = 0;
    for (uint32_t l = 1, c = 0; l <= max_len; ++l) { c = (c + count[l - 1]) << 1; next[l] = c; }
    for (uint32_t s = 0; s < n_sym; ++s) {
        uint32_t c = len[s] ? next[len[s]]++ : 0u, r = 0;
        for (uint32_t k = 0; k < len[s]; ++k) { r = (r << 1) | (c & 1u); c >>= 1; }
        code[s] = (uint16_t)r;
    }
}
struct GzBits {
    uint8_t *p; uint32_t n;
    void put(uint32_t v, uint32_t bits) { for (uint32_t k = 0; k < bits; ++k, ++n) p[n >> 3] |= (uint8_t)(((v >> k) & 1u) << (n & 7u)); }
};
static inline int gz_code_build(const uint64_t hist[256], ns_gz_code *out) {
    if (!hist || !out) return NS_EINVAL;
    memset(out, 0, sizeof *out);
    uint64_t freq[257];
    for (uint32_t v = 0; v < 256; ++v) freq[v] = hist[v];
    freq[GZ_EOB] = 1;                                                // every block ends with one
    gz_huff_lengths(freq, 257, 15, out->len);
    gz_canonical(out->len, 257, 15, out->code);
    // the 258 lengths (257 literal/length codes and one distance code of length 0) in the code-length alphabet: 16 repeats the last
    // length 3-6 times, 17 stands for 3-10 zeros, 18 for 11-138
    uint8_t lens[258], tok[258], ext[258];
    uint32_t n_tok = 0;
    memcpy(lens, out->len, 257); lens[257] = 0;
    for (uint32_t i = 0; i < 258;) {
        uint32_t run = 1;
        while (i + run < 258 && lens[i + run] == lens[i]) ++run;
        uint32_t left = run;
        if (!lens[i]) {
            while (left >= 11) { const uint32_t r = left < 138 ? left : 138; tok[n_tok] = 18; ext[n_tok++] = (uint8_t)(r - 11); left -= r; }
            if (left >= 3) { tok[n_tok] = 17; ext[n_tok++] = (uint8_t)(left - 3); left = 0; }
        } else {
            tok[n_tok] = lens[i]; ext[n_tok++] = 0; left--;
            while (left >= 3) { const uint32_t r = left < 6 ? left : 6; tok[n_tok] = 16; ext[n_tok++] = (uint8_t)(r - 3); left -= r; }
        }
        for (; left; --left) { tok[n_tok] = lens[i]; ext[n_tok++] = 0; }
        i += run;
    }
    uint64_t cl_freq[19] = {0};
    uint8_t cl_len[19]; uint16_t cl_code[19];
    uint32_t cl_used = 0;
    for (uint32_t t = 0; t < n_tok; ++t) cl_freq[tok[t]]++;
    for (uint32_t s = 0; s < 19; ++s) cl_used += cl_freq[s] != 0;
    if (cl_used == 1) cl_freq[cl_freq[0] ? 1 : 0] = 1;               // (inflate wants a complete code-length code: a second symbol, never used.  Not reached from here: end-of-block's length and the 0 of the distance code are always two tokens)
    gz_huff_lengths(cl_freq, 19, 7, cl_len);
    gz_canonical(cl_len, 19, 7, cl_code);
    static const uint8_t cl_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    uint32_t hclen = 4;
    for (uint32_t k = 0; k < 19; ++k) if (cl_len[cl_order[k]] && k + 1 > hclen) hclen = k + 1;
    GzBits b{out->header, 0};
    b.put(1, 1); b.put(2, 2); b.put(0, 5); b.put(0, 5); b.put(hclen - 4, 4);
    for (uint32_t k = 0; k < hclen; ++k) b.put(cl_len[cl_order[k]], 3);
    for (uint32_t t = 0; t < n_tok; ++t) {
        b.put(cl_code[tok[t]], cl_len[tok[t]]);
        if (tok[t] >= 16) b.put(ext[t], tok[t] == 16 ? 2 : tok[t] == 17 ? 3 : 7);
    }
    out->header_bits = b.n;
    return b.n <= GZ_HEADER_BITS_MAX ? NS_OK : NS_EINVAL;            // (cannot happen: the bound is derived in include/nanosim_amd.h)
}
// a code somebody else filled in: every length a deflate length, the header within its array
static inline bool gz_code_valid(const ns_gz_code *c) {
    for (uint32_t v = 0; v < 257; ++v) if (c->len[v] > 15 || (c->len[v] && (c->code[v] >> c->len[v]))) return false;
    return c->len[GZ_EOB] != 0 && c->header_bits >= 17u && c->header_bits <= GZ_HEADER_BITS_MAX;
}
static inline uint32_t gz_mulx(uint32_t p) { return (p >> 1) ^ ((p & 1u) ? GZ_CRC_POLY : 0u); }          // p * x mod P
static inline void gz_dev_code(const ns_gz_code *c, GzDevCode *d) {
    for (uint32_t v = 0; v < 257; ++v) d->sym[v] = (uint32_t)c->len[v] << 16 | c->code[v];
    d->header_bits = c->header_bits;
    memcpy(d->header, c->header, NS_GZ_HEADER_BYTES);
    uint32_t p = 0x80000000u;                                        // x^0
    for (uint32_t l = GZ_LANES; l-- > 0;) { d->lane_pow[l] = p; for (uint32_t k = 0; k < 8u * GZ_SPAN; ++k) p = gz_mulx(p); }
    for (uint32_t v = 0; v < 256; ++v) { uint32_t r = v; for (int k = 0; k < 8; ++k) r = gz_mulx(r); d->crc_tab[v] = r; }
}
static inline uint64_t gz_bound(uint64_t nbytes, uint32_t n_ranges) {
    return nbytes + (uint64_t)(GZ_MEMBER_EXTRA + GZ_STORED_EXTRA) * (nbytes / NS_GZ_BLOCK_BYTES + n_ranges);
}

// ---------------------------------------------------------------------------------------------------------
// the walk: one wavefront, one member.  W: lane, scan (exclusive prefix sum + total, 32 bits), ballot, shfl, fence
// ---------------------------------------------------------------------------------------------------------
NS_CSH uint32_t gz_mulmod(uint32_t a, uint32_t b) {                  // a * b mod P, both reflected (bit 31: x^0)
    uint32_t p = 0;
    for (uint32_t m = 0x80000000u; m; m >>= 1) { if (a & m) p ^= b; b = (b >> 1) ^ ((b & 1u) ? GZ_CRC_POLY : 0u); }
    return p;
}
// the bytes [lo, hi) of the block that lane `lane` carries (hi == 0: none)
NS_CSH void gz_span(uint32_t lane, uint32_t n, uint32_t &lo, uint32_t &hi) {
    const uint32_t gap = NS_GZ_BLOCK_BYTES - n, g0 = lane * GZ_SPAN, g1 = g0 + GZ_SPAN;
    lo = g0 > gap ? g0 - gap : 0u;
    hi = g1 > gap ? g1 - gap : 0u;
}
// f(byte) for p[lo .. hi): single bytes up to a word boundary of the address, aligned words, single bytes
template <class F> NS_CSH void gz_each(const uint8_t *p, uint32_t lo, uint32_t hi, F &&f) {
    uint32_t i = lo;
    for (; i < hi && ((uintptr_t)(p + i) & 3u); ++i) f((uint32_t)p[i]);
    for (; i + 4u <= hi; i += 4u) {
        uint32_t v;
        __builtin_memcpy(&v, __builtin_assume_aligned(p + i, 4), 4);
        f(v & 0xffu); f((v >> 8) & 0xffu); f((v >> 16) & 0xffu); f(v >> 24);
    }
    for (; i < hi; ++i) f((uint32_t)p[i]);
}
struct GzLay {
    bool stored;
    uint32_t ex;                     // the bits of the lanes in front of this one
    uint32_t head_bits;              // the bits of the block header
    uint32_t member;                 // the bytes of the member
};
// what the member of src[0 .. n) looks like (1 <= n <= NS_GZ_BLOCK_BYTES); CRC: and this lane's CRC register over its span
template <bool CRC, class W> NS_CSH GzLay gz_layout(W &w, const GzTabs &T, const uint8_t *src, uint32_t n, uint32_t &crc_reg) {
    uint32_t lo, hi;
    gz_span(w.lane, n, lo, hi);
    const bool first = hi && !lo;
    uint32_t bits = 0, miss = 0, r = first ? 0xffffffffu : 0u;
    gz_each(src, lo, hi, [&](uint32_t b) {
        const uint32_t l = T.sym[b] >> 16;
        bits += l; miss |= l ? 0u : 1u;
        if (CRC) r = T.crc_tab[(r ^ b) & 0xffu] ^ (r >> 8);
    });
    crc_reg = r;
    uint32_t total;
    const uint32_t ex = w.scan(bits, total);
    const bool lacks = w.ballot(miss != 0u) != 0ull;
    const uint32_t coded = (T.header_bits + total + (T.sym[GZ_EOB] >> 16) + 7u) >> 3, raw = GZ_STORED_EXTRA + n;
    GzLay L;
    L.stored = lacks || coded > raw;
    L.ex = L.stored ? 8u * lo : ex;
    L.head_bits = L.stored ? 8u * GZ_STORED_EXTRA : T.header_bits;
    L.member = GZ_MEMBER_EXTRA + (L.stored ? raw : coded);
    return L;
}
template <class W> NS_CSH uint32_t gz_member_size(W &w, const GzTabs &T, const uint8_t *src, uint32_t n) {
    uint32_t r;
    return gz_layout<false>(w, T, src, n, r).member;
}
// word i of the block header's bit string, zeros behind it
NS_CSH uint32_t gz_head_word(const GzTabs &T, bool stored, uint32_t n, uint32_t i) {
    if (stored) { const uint32_t nl = ~n & 0xffffu; return i == 0u ? (1u | n << 8 | (nl & 0xffu) << 24) : i == 1u ? nl >> 8 : 0u; }
    return i < GZ_HEADER_WORDS ? T.header[i] : 0u;
}
// word i of the prefix: the BGZF header (1f 8b 08 04, MTIME 0, XFL 0, OS ff, XLEN 6, 'B' 'C' 2 0, BSIZE - 1), then the block header
NS_CSH uint32_t gz_prefix_word(const GzTabs &T, bool stored, uint32_t n, uint32_t member, uint32_t i) {
    switch (i) {
        case 0u: return 0x04088b1fu;
        case 1u: return 0u;
        case 2u: return 0x0006ff00u;
        case 3u: return 0x00024342u;
        case 4u: return (member - 1u) | gz_head_word(T, stored, n, 0u) << 16;
        default: return gz_head_word(T, stored, n, i - 5u) >> 16 | gz_head_word(T, stored, n, i - 4u) << 16;
    }
}
struct GzAcc {                       // a lane's bit accumulator and the word it is filling
    uint64_t acc; uint32_t nb, wi, frag; bool give;
    uint32_t *stage;
};
// the accumulator's low word is complete: it goes to its place — or, the bits in front of the lane's first word boundary, to `frag`
NS_CSH void gz_flush(GzAcc &a) {
    if (a.give) { a.frag = (uint32_t)a.acc; a.give = false; } else a.stage[a.wi] = (uint32_t)a.acc;
    ++a.wi; a.acc >>= 32; a.nb -= 32u;
}
NS_CSH void gz_put(GzAcc &a, uint32_t v, uint32_t bits) {            // bits <= 32, a.nb < 32
    a.acc |= (uint64_t)v << a.nb; a.nb += bits;
    if (a.nb >= 32u) gz_flush(a);
}
// the member of src[0 .. n) to dst[0 .. expect), through stage[GZ_STAGE_WORDS]; expect: what gz_member_size gave.  Returns the member's
// size; when that is not `expect`, nothing was stored to dst
template <class W> NS_CSH uint32_t gz_member(W &w, const GzTabs &T, const uint8_t *src, uint32_t n, uint32_t *stage, uint8_t *dst, uint32_t expect) {
    uint32_t r;
    const GzLay L = gz_layout<true>(w, T, src, n, r);
    r = gz_mulmod(r, T.lane_pow[w.lane]);
    for (uint32_t o = 1u; o < GZ_LANES; o <<= 1) r ^= w.shfl(r, w.lane ^ o);
    const uint32_t crc = ~r;
    if (L.member != expect) return L.member;
    const uint32_t prefix_bits = GZ_BGZF_BITS + L.head_bits, pw = prefix_bits >> 5, pr = prefix_bits & 31u;
    if (w.lane < pw) stage[w.lane] = gz_prefix_word(T, L.stored, n, L.member, w.lane);
    uint32_t lo, hi;
    gz_span(w.lane, n, lo, hi);
    GzAcc a{0ull, 0u, 0u, 0u, false, stage};
    if (hi) {
        if (!lo) { a.wi = pw; a.nb = pr; a.acc = gz_prefix_word(T, L.stored, n, L.member, pw) & ((1u << pr) - 1u); }
        else { const uint32_t p = prefix_bits + L.ex; a.wi = p >> 5; a.nb = p & 31u; a.give = a.nb != 0u; }
        const bool stored = L.stored;
        gz_each(src, lo, hi, [&](uint32_t b) {
            const uint32_t s = stored ? (8u << 16 | b) : T.sym[b];
            gz_put(a, s & 0xffffu, s >> 16);
        });
        if (w.lane == GZ_LANES - 1u) {
            if (!stored) gz_put(a, T.sym[GZ_EOB] & 0xffffu, T.sym[GZ_EOB] >> 16);
            a.nb = (a.nb + 7u) & ~7u;
            if (a.nb >= 32u) gz_flush(a);
            gz_put(a, crc, 32u); gz_put(a, n, 32u);
            if (a.nb) stage[a.wi] = (uint32_t)a.acc;
            a.nb = 0u;
        }
    }
    const uint32_t frag = w.shfl(a.frag, w.lane + 1u);               // the bits that complete my last word (the last lane has none left)
    if (hi && a.nb) stage[a.wi] = (uint32_t)a.acc | frag;
    w.fence();
    // the staging image to its place
    const uint8_t *sb = reinterpret_cast<const uint8_t *>(stage);
    uint32_t head = (uint32_t)((4u - ((uintptr_t)dst & 3u)) & 3u);
    if (head > L.member) head = L.member;
    if (w.lane < head) dst[w.lane] = sb[w.lane];
    const uint32_t words = (L.member - head) >> 2, sh = 8u * head;
    for (uint32_t k = w.lane; k < words; k += GZ_LANES) {
        const uint32_t v = sh ? (stage[k] >> sh | stage[k + 1u] << (32u - sh)) : stage[k];
        __builtin_memcpy(__builtin_assume_aligned(dst + head + 4u * k, 4), &v, 4);
    }
    for (uint32_t j = head + 4u * words + w.lane; j < L.member; j += GZ_LANES) dst[j] = sb[j];
    return L.member;
}
// the blocks of a call (host and device: tests/gz_wave_host.cpp walks them on the CPU): range r = [cuts[r], cuts[r + 1]) has the blocks first[r] .. first[r + 1), NS_GZ_BLOCK_BYTES each but the last
struct GzBlocks { const unsigned long long *cuts; const uint32_t *first; uint32_t n_ranges, n_blk; };
NS_CSH void gz_block_at(const GzBlocks &B, uint32_t g, uint64_t &off, uint32_t &n) {
    uint32_t lo = 0, hi = B.n_ranges - 1u;                           // the last range whose first block is not behind g
    while (lo < hi) { const uint32_t mid = lo + (hi - lo + 1u) / 2u; if (B.first[mid] <= g) lo = mid; else hi = mid - 1u; }
    off = B.cuts[lo] + (uint64_t)(g - B.first[lo]) * NS_GZ_BLOCK_BYTES;
    const uint64_t left = B.cuts[lo + 1u] - off;
    n = left < NS_GZ_BLOCK_BYTES ? (uint32_t)left : NS_GZ_BLOCK_BYTES;
}

// ---------------------------------------------------------------------------------------------------------
// the kernels
// ---------------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)
#define GZ_WAVES 2u                  // wavefronts (members) per workgroup of the two block kernels: 2 x 16.4 KB of staging + 2 KB of tables
struct GzWaveDev {
    static constexpr uint32_t LANES = 64u;
    uint32_t lane;
    __device__ __forceinline__ uint32_t scan(uint32_t v, uint32_t &total) const {
        uint32_t incl = v;
        for (int o = 1; o < 64; o <<= 1) { const uint32_t u = (uint32_t)__shfl_up((int)incl, o, 64); if (lane >= (uint32_t)o) incl += u; }
        total = (uint32_t)__shfl((int)incl, 63, 64);
        return incl - v;
    }
    __device__ __forceinline__ uint64_t ballot(bool pred) const { return __ballot(pred); }
    __device__ __forceinline__ uint32_t shfl(uint32_t v, uint32_t src) const { return (uint32_t)__shfl((int)v, (int)(src & 63u), 64); }
    __device__ __forceinline__ void fence() const { __threadfence_block(); }
};
// the counts of the byte values of src[0 .. n): 256 counters per workgroup in LDS, one global add per counter and workgroup.  src is
// 4-byte aligned; every workgroup takes whole words at a grid stride, the last bytes go to the first thread
__global__ void __launch_bounds__(256) k_gz_hist(const uint8_t *__restrict__ src, uint64_t n, unsigned long long *__restrict__ hist) {
    __shared__ uint32_t cnt[256];
    cnt[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t words = n >> 2, stride = (uint64_t)gridDim.x * 256u;
    const uint32_t *w = reinterpret_cast<const uint32_t *>(src);
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < words; i += stride) {
        const uint32_t v = w[i];
        atomicAdd(&cnt[v & 0xffu], 1u); atomicAdd(&cnt[(v >> 8) & 0xffu], 1u); atomicAdd(&cnt[(v >> 16) & 0xffu], 1u); atomicAdd(&cnt[v >> 24], 1u);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) for (uint64_t i = words << 2; i < n; ++i) atomicAdd(&cnt[src[i]], 1u);
    __syncthreads();
    if (cnt[threadIdx.x]) atomicAdd(&hist[threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
}
// SIZE: size[g] = the bytes of block g's member.  Reads the input, writes nothing else
__global__ void __launch_bounds__(64 * GZ_WAVES) k_gz_size(const uint8_t *__restrict__ src, GzBlocks B, const GzDevCode *__restrict__ code,
                                                           unsigned long long *__restrict__ size) {
    __shared__ uint32_t sym[257];
    for (uint32_t i = threadIdx.x; i < 257u; i += 64u * GZ_WAVES) sym[i] = code->sym[i];
    __syncthreads();
    const uint32_t g = blockIdx.x * GZ_WAVES + (threadIdx.x >> 6);
    if (g >= B.n_blk) return;                                        // (a whole wavefront leaves)
    GzWaveDev w{threadIdx.x & 63u};
    const GzTabs T{sym, nullptr, code->header, code->lane_pow, code->header_bits};
    uint64_t off; uint32_t n;
    gz_block_at(B, g, off, n);
    const uint32_t m = gz_member_size(w, T, src + off, n);
    if (w.lane == 0) size[g] = m;
}
// EMIT, behind the exclusive scan of the sizes: block g's member at dst + at[g].  A member that is not what SIZE measured is not stored
// and counts in *mismatch
__global__ void __launch_bounds__(64 * GZ_WAVES) k_gz_emit(const uint8_t *__restrict__ src, GzBlocks B, const GzDevCode *__restrict__ code,
                                                           const unsigned long long *__restrict__ at, uint8_t *__restrict__ dst,
                                                           unsigned long long *__restrict__ mismatch) {
    __shared__ uint32_t sym[257], crc_tab[256];
    __shared__ uint32_t stage[GZ_WAVES][GZ_STAGE_WORDS];
    for (uint32_t i = threadIdx.x; i < 257u; i += 64u * GZ_WAVES) sym[i] = code->sym[i];
    for (uint32_t i = threadIdx.x; i < 256u; i += 64u * GZ_WAVES) crc_tab[i] = code->crc_tab[i];
    __syncthreads();
    const uint32_t g = blockIdx.x * GZ_WAVES + (threadIdx.x >> 6);
    if (g >= B.n_blk) return;
    GzWaveDev w{threadIdx.x & 63u};
    const GzTabs T{sym, crc_tab, code->header, code->lane_pow, code->header_bits};
    uint64_t off; uint32_t n;
    gz_block_at(B, g, off, n);
    const uint32_t expect = (uint32_t)(at[g + 1u] - at[g]);
    const uint32_t m = gz_member(w, T, src + off, n, stage[threadIdx.x >> 6], dst + at[g], expect);
    if (m != expect && w.lane == 0) atomicAdd(mismatch, 1ull);
}
// where the members of every range begin: gz_off[i] = at[first[i]], i <= n_ranges
__global__ void __launch_bounds__(256) k_gz_offsets(const uint32_t *__restrict__ first, uint32_t n_cuts, const unsigned long long *__restrict__ at,
                                                    unsigned long long *__restrict__ gz_off) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_cuts) gz_off[i] = at[first[i]];
}
#endif
