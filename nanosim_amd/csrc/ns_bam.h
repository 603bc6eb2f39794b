// ns_bam.h — training side, BAM records to SAM text ("BAM input"): what `samtools view` prints for the records of a BAM file,
// byte for byte, from the inflated bytes of the file.  The reference reads BAM through pysam everywhere (src/read_analysis.py:84,136,170);
// the stages here read SAM text, so the decode to text is the one piece that reaches all of them.
//
// A record (all little-endian): block_size i32 | refID i32 | pos i32 | l_read_name u8 | mapq u8 | bin u16 | n_cigar_op u16 | flag u16 |
// l_seq i32 | next_refID i32 | next_pos i32 | tlen i32 | name (NUL included) | cigar u32[n] (len << 4 | op) | seq u8[(l_seq + 1) / 2]
// (high nibble first) | qual u8[l_seq] | tags up to block_size.
//
// Two walks per record, both by ONE WAVEFRONT (W::LANES lanes; the host build runs the same code with one lane):
//   measure  (bam_measure) validates the record and computes the length of its line.  The header counts give most lengths; the CIGAR's
//            digit counts are summed BAM_ROUND_OPS ops at a time, a Z / H tag's length is found BAM_STRLEN_BYTES per lane at a time, the
//            elements of an integer B array like the CIGAR's ops.  Where a float stands (type f, elements of B:f) goes to a list: their
//            text is made by the host's C library ("%g") and comes back in slots of BAM_FLOAT_SLOT bytes, in the order of the records.
//            Long CIGARs (htslib's rule): when the first op is `S` with length l_seq and a CG:B:I tag is present, the CIGAR is the tag's
//            array and the tag is not printed.
//   write    (bam_write) one wavefront per SLICE of a record: slice k holds bases k * BAM_SLICE_BASES .. of SEQ and of QUAL, slice 0
//            everything else.  The bulk fields — SEQ (nibble decode), QUAL (+33), names and Z / H values (copies) — go through
//            bam_bulk: the lanes stride over pieces of BAM_LANE_BYTES output bytes that are aligned in the TEXT, one 16-byte store each,
//            with single bytes in front of the first and behind the last piece.  CIGAR ops and B elements go W::LANES at a time, placed
//            by a prefix sum of their lengths over the wavefront.  The small fields are written by lane 0.
// Every load lies inside the record (`end` = its block_size, which the caller has checked against the buffer), every store inside the
// line (the cursor is checked against the measured length in front of every field; bam_write returns false when the two walks disagree).
// W, the wavefront: lane, scan (exclusive prefix sum + total), first (lowest lane with a predicate), bcast, float_reserve / float_put.
#pragma once
#include <stdint.h>
#include "ns_cs_hist.h"

#define BAM_ROUND_OPS 64u            // CIGAR ops / B-array elements per round of a wavefront (its lanes)
#define BAM_LANE_BYTES 16u           // output bytes per lane and pass of the bulk fields: one aligned 16-byte store
#define BAM_SLICE_BASES 4096u        // bases of SEQ and of QUAL per slice of a record (even: a slice begins at a whole SEQ byte)
#define BAM_STRLEN_BYTES 8u          // bytes a lane looks at per round of the search for a Z / H tag's NUL
#define BAM_FLOAT_SLOT 16u           // the text of one float: at most BAM_FLOAT_CHARS characters, their number in the last byte
#define BAM_FLOAT_CHARS 12u          // "-1.17549e-38"
#define BAM_FIXED 32u                // the bytes of a record between block_size and the name

enum { BAM_OK = 0, BAM_BAD_BLOCK_SIZE = 1, BAM_BAD_LSEQ = 2, BAM_BAD_REFID = 3, BAM_BAD_NAME = 4, BAM_BAD_TAG_TYPE = 5, BAM_BAD_TAG_NUL = 6,
       BAM_BAD_TAG_COUNT = 7, BAM_BAD_TRUNCATED = 8 };
enum { BAM_COPY = 0, BAM_PLUS33 = 1, BAM_NIBBLE = 2 };

struct BamRefs { const uint8_t *names; const uint64_t *off; uint32_t n_ref; };     // name i: names[off[i] .. off[i + 1])
struct BamRec {                      // what the write pass takes over from the measure pass
    uint64_t cigar_at;               // where the ops stand: in the record, or in its CG tag
    uint64_t cg_at;                  // the first byte of the CG tag that is not printed; ~0 without
    uint64_t seq_at;                 // the offset of SEQ in the line
    uint64_t cigar_len;              // the bytes of the CIGAR's text
    uint32_t n_cigar, reserved;
};
struct alignas(16) BamPiece { uint64_t lo, hi; };

NS_CSH uint32_t bam_u16(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
NS_CSH uint32_t bam_u32(const uint8_t *p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }
NS_CSH uint64_t bam_u64(const uint8_t *p) { uint64_t v; __builtin_memcpy(&v, p, 8); return v; }
NS_CSH uint32_t bam_dec_len(uint32_t v) {
    return 1u + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) + (v >= 10000000u) + (v >= 100000000u) +
           (v >= 1000000000u);
}
NS_CSH void bam_put_dec(uint8_t *dst, uint32_t v, uint32_t n) { for (uint32_t i = n; i-- > 0;) { dst[i] = (uint8_t)('0' + v % 10u); v /= 10u; } }
// a signed value as (sign, magnitude): everything a record prints has 32 bits, or is one more than such a value
NS_CSH uint32_t bam_mag(int64_t v, uint32_t &neg) { neg = v < 0 ? 1u : 0u; return (uint32_t)(v < 0 ? -v : v); }
NS_CSH uint32_t bam_sdec_len(int64_t v) { uint32_t neg; const uint32_t m = bam_mag(v, neg); return neg + bam_dec_len(m); }
NS_CSH uint32_t bam_put_sdec(uint8_t *dst, int64_t v) {
    uint32_t neg; const uint32_t m = bam_mag(v, neg), n = bam_dec_len(m);
    if (neg) dst[0] = '-';
    bam_put_dec(dst + neg, m, n);
    return neg + n;
}
// entry i of a table of 16 characters kept in two words
NS_CSH uint8_t bam_pick16(uint64_t lo, uint64_t hi, uint32_t i) { return (uint8_t)(((i & 8u) ? hi : lo) >> (8u * (i & 7u))); }
NS_CSH uint8_t bam_seq_char(uint32_t nib) { return bam_pick16(0x565352474d43413dull, 0x4e42444b48595754ull, nib); }      // "=ACMGRSVTWYHKDBN"
NS_CSH uint8_t bam_op_char(uint32_t op) { return bam_pick16(0x3d5048534e44494dull, 0x3f3f3f3f3f3f3f58ull, op); }        // "MIDNSHP=X???????"
NS_CSH uint32_t bam_type_size(uint8_t t) {
    return (t == 'A' || t == 'c' || t == 'C') ? 1u : (t == 's' || t == 'S') ? 2u : (t == 'i' || t == 'I' || t == 'f') ? 4u : 0u;
}
NS_CSH int64_t bam_int_at(const uint8_t *p, uint8_t type) {          // c C s S i I, signed or unsigned as stored
    switch (type) {
        case 'c': return (int8_t)p[0];
        case 'C': return p[0];
        case 's': return (int16_t)bam_u16(p);
        case 'S': return bam_u16(p);
        case 'i': return (int32_t)bam_u32(p);
        default: return bam_u32(p);
    }
}

// ---- the bulk fields ----
template <int KIND> NS_CSH uint8_t bam_bulk_byte(const uint8_t *src, uint64_t j) {
    if (KIND == BAM_NIBBLE) { const uint32_t b = src[j >> 1]; return bam_seq_char((j & 1u) ? (b & 15u) : (b >> 4)); }
    return KIND == BAM_PLUS33 ? (uint8_t)(src[j] + 33u) : src[j];
}
NS_CSH uint64_t bam_plus33(uint64_t x) {                             // + 33 on each of eight bytes, each modulo 256
    const uint64_t H = 0x8080808080808080ull;
    return ((x & ~H) + 0x2121212121212121ull) ^ (x & H);
}
// output bytes j0 .. j0 + 15 of a field (all of them exist)
template <int KIND> NS_CSH BamPiece bam_bulk_piece(const uint8_t *src, uint64_t j0) {
    BamPiece o;
    if (KIND == BAM_NIBBLE) {
        const uint64_t k0 = j0 >> 1;
        const uint32_t odd = (uint32_t)(j0 & 1u);
        const uint64_t v = bam_u64(src + k0);
        const uint32_t b8 = odd ? src[k0 + 8u] : 0u;                 // (an odd start ends in the high nibble of a ninth byte)
        o.lo = o.hi = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (uint32_t i = 0; i < 16u; ++i) {
            const uint32_t idx = i + odd, by = idx >> 1;
            const uint32_t byte = by < 8u ? (uint32_t)(v >> (8u * by)) & 0xffu : b8;
            const uint64_t c = bam_seq_char((idx & 1u) ? (byte & 15u) : (byte >> 4));
            if (i < 8u) o.lo |= c << (8u * i); else o.hi |= c << (8u * (i - 8u));
        }
    } else {
        o.lo = bam_u64(src + j0); o.hi = bam_u64(src + j0 + 8u);
        if (KIND == BAM_PLUS33) { o.lo = bam_plus33(o.lo); o.hi = bam_plus33(o.hi); }
    }
    return o;
}
// n output bytes of a field to dst: single bytes up to the first 16-byte boundary of the text, aligned pieces, single bytes behind them
template <int KIND, class W> NS_CSH void bam_bulk(W &w, const uint8_t *src, uint64_t n, uint8_t *dst) {
    uint64_t head = (uint64_t)((BAM_LANE_BYTES - ((uintptr_t)dst & (BAM_LANE_BYTES - 1u))) & (BAM_LANE_BYTES - 1u));
    if (head > n) head = n;
    for (uint64_t j = w.lane; j < head; j += W::LANES) dst[j] = bam_bulk_byte<KIND>(src, j);
    const uint64_t pieces = (n - head) / BAM_LANE_BYTES;
    for (uint64_t c = w.lane; c < pieces; c += W::LANES) {
        const uint64_t j0 = head + c * BAM_LANE_BYTES;
        *reinterpret_cast<BamPiece *>(dst + j0) = bam_bulk_piece<KIND>(src, j0);
    }
    for (uint64_t j = head + pieces * BAM_LANE_BYTES + w.lane; j < n; j += W::LANES) dst[j] = bam_bulk_byte<KIND>(src, j);
}

// ---- the tags ----
// the length of the NUL-terminated string at `at`; false: no NUL in front of `end`
template <class W> NS_CSH bool bam_strlen(W &w, const uint8_t *b, uint64_t at, uint64_t end, uint64_t &len) {
    for (uint64_t base = at; base < end; base += (uint64_t)BAM_STRLEN_BYTES * W::LANES) {
        const uint64_t p = base + (uint64_t)BAM_STRLEN_BYTES * w.lane;
        uint32_t z = BAM_STRLEN_BYTES;                               // the first NUL among my bytes; BAM_STRLEN_BYTES: none
        if (p + BAM_STRLEN_BYTES <= end) {
            const uint64_t v = bam_u64(b + p), m = (v - 0x0101010101010101ull) & ~v & 0x8080808080808080ull;
            if (m) z = (uint32_t)__builtin_ctzll(m) >> 3;
        } else {
            for (uint32_t k = 0; k < BAM_STRLEN_BYTES && p + k < end; ++k) if (!b[p + k]) { z = k; break; }
        }
        const uint32_t l = w.first(z < BAM_STRLEN_BYTES);
        if (l < W::LANES) { len = (base - at) + (uint64_t)BAM_STRLEN_BYTES * l + w.bcast(z, l); return true; }
    }
    return false;
}
struct BamTag {
    uint8_t type, sub;               // sub: the element type of a B array
    uint32_t count;                  // B: elements
    uint64_t val_at, len, next;      // the value (B: its first element); Z / H: its length; the tag behind
};
// the tag at `at` (< end); BAM_OK or why the record is bad
template <class W> NS_CSH uint32_t bam_next_tag(W &w, const uint8_t *b, uint64_t at, uint64_t end, BamTag &t) {
    t.sub = 0; t.count = 0; t.len = 0;
    if (end - at < 3u) return BAM_BAD_TAG_COUNT;
    t.type = b[at + 2u];
    t.val_at = at + 3u;
    const uint32_t size = bam_type_size(t.type);
    if (size) {
        if (end - t.val_at < size) return BAM_BAD_TAG_COUNT;
        t.next = t.val_at + size;
    } else if (t.type == 'Z' || t.type == 'H') {
        if (!bam_strlen(w, b, t.val_at, end, t.len)) return BAM_BAD_TAG_NUL;
        t.next = t.val_at + t.len + 1u;
    } else if (t.type == 'B') {
        if (end - t.val_at < 5u) return BAM_BAD_TAG_COUNT;
        t.sub = b[t.val_at];
        t.count = bam_u32(b + t.val_at + 1u);
        t.val_at += 5u;
        const uint32_t es = t.sub == 'A' ? 0u : bam_type_size(t.sub);
        if (!es) return BAM_BAD_TAG_TYPE;
        if ((uint64_t)t.count * es > end - t.val_at) return BAM_BAD_TAG_COUNT;
        t.next = t.val_at + (uint64_t)t.count * es;
    } else return BAM_BAD_TAG_TYPE;
    return BAM_OK;
}
// the text of CIGAR ops: its length, and (write) the text itself
template <bool WRITE, class W> NS_CSH uint64_t bam_cigar_text(W &w, const uint8_t *ops, uint32_t n, uint8_t *dst) {
    uint64_t total = 0;
    for (uint64_t base = 0; base < n; base += W::LANES) {
        const uint64_t i = base + w.lane;
        uint32_t v = 0, l = 0, t;
        if (i < n) { v = bam_u32(ops + 4u * i); l = bam_dec_len(v >> 4) + 1u; }
        const uint32_t ex = w.scan(l, t);
        if (WRITE && i < n) { uint8_t *q = dst + total + ex; bam_put_dec(q, v >> 4, l - 1u); q[l - 1u] = bam_op_char(v & 15u); }
        total += t;
    }
    return total;
}
// the text of the elements of an integer B array, ",v" each
template <bool WRITE, class W> NS_CSH uint64_t bam_b_text(W &w, const uint8_t *p, uint8_t sub, uint32_t count, uint8_t *dst) {
    const uint32_t es = bam_type_size(sub);
    uint64_t total = 0;
    for (uint64_t base = 0; base < count; base += W::LANES) {
        const uint64_t i = base + w.lane;
        int64_t v = 0;
        uint32_t l = 0, t;
        if (i < count) { v = bam_int_at(p + i * es, sub); l = 1u + bam_sdec_len(v); }
        const uint32_t ex = w.scan(l, t);
        if (WRITE && i < count) { uint8_t *q = dst + total + ex; q[0] = ','; bam_put_sdec(q + 1, v); }
        total += t;
    }
    return total;
}
// the text of the elements of a B:f array from their slots, ",v" each
template <bool WRITE, class W> NS_CSH uint64_t bam_bf_text(W &w, const uint8_t *slots, uint32_t count, uint8_t *dst) {
    uint64_t total = 0;
    for (uint64_t base = 0; base < count; base += W::LANES) {
        const uint64_t i = base + w.lane;
        uint32_t l = 0, t;
        const uint8_t *s = slots + i * BAM_FLOAT_SLOT;
        if (i < count) { l = s[BAM_FLOAT_SLOT - 1u]; if (l > BAM_FLOAT_CHARS) l = BAM_FLOAT_CHARS; l += 1u; }
        const uint32_t ex = w.scan(l, t);
        if (WRITE && i < count) { uint8_t *q = dst + total + ex; q[0] = ','; for (uint32_t k = 1; k < l; ++k) q[k] = s[k - 1u]; }
        total += t;
    }
    return total;
}

struct BamHead {                     // the fixed fields of a record
    int32_t ref_id, pos, l_seq, next_ref, next_pos, tlen;
    uint32_t l_name, mapq, n_cigar, flag;
};
NS_CSH void bam_head(const uint8_t *f, BamHead &h) {                 // f: behind block_size
    h.ref_id = (int32_t)bam_u32(f); h.pos = (int32_t)bam_u32(f + 4); h.l_name = f[8]; h.mapq = f[9]; h.n_cigar = bam_u16(f + 12);
    h.flag = bam_u16(f + 14); h.l_seq = (int32_t)bam_u32(f + 16); h.next_ref = (int32_t)bam_u32(f + 20); h.next_pos = (int32_t)bam_u32(f + 24);
    h.tlen = (int32_t)bam_u32(f + 28);
}
NS_CSH uint64_t bam_ref_len(const BamRefs &R, int32_t id) { return id < 0 ? 1u : R.off[id + 1] - R.off[id]; }
// the offset of SEQ in the line: the nine fields in front of it with their tabs
NS_CSH uint64_t bam_seq_at(const BamHead &h, const BamRefs &R, uint64_t cigar_len) {
    return (uint64_t)(h.l_name - 1u) + 1u + bam_dec_len(h.flag) + 1u + bam_ref_len(R, h.ref_id) + 1u + bam_sdec_len((int64_t)h.pos + 1) + 1u +
           bam_dec_len(h.mapq) + 1u + cigar_len + 1u + ((h.next_ref >= 0 && h.next_ref == h.ref_id) ? 1u : bam_ref_len(R, h.next_ref)) + 1u +
           bam_sdec_len((int64_t)h.next_pos + 1) + 1u + bam_sdec_len(h.tlen) + 1u;
}

// ---- measure: the record at bytes[at .. end) (at: its block_size field; end = at + 4 + block_size) ----
// BAM_OK: rec, line_len (floats not counted), n_slices, n_float (the floats whose places went to the list); else why it is bad
template <class W> NS_CSH uint32_t bam_measure(W &w, const uint8_t *b, uint64_t at, uint64_t end, const BamRefs &R, BamRec &rec, uint64_t &line_len,
                                               uint32_t &n_slices) {
    if (end - at < 4u + BAM_FIXED) return BAM_BAD_BLOCK_SIZE;
    BamHead h;
    bam_head(b + at + 4u, h);
    if (h.l_seq < 0) return BAM_BAD_LSEQ;
    const uint64_t l_seq = (uint64_t)h.l_seq, name_at = at + 4u + BAM_FIXED, cigar_at = name_at + h.l_name, seq_at = cigar_at + 4ull * h.n_cigar,
                   qual_at = seq_at + (l_seq + 1u) / 2u, tags_at = qual_at + l_seq;
    if (tags_at > end) return BAM_BAD_BLOCK_SIZE;
    if (h.ref_id < -1 || h.next_ref < -1 || (h.ref_id >= 0 && (uint32_t)h.ref_id >= R.n_ref) || (h.next_ref >= 0 && (uint32_t)h.next_ref >= R.n_ref))
        return BAM_BAD_REFID;
    if (!h.l_name || b[cigar_at - 1u]) return BAM_BAD_NAME;
    rec.cigar_at = cigar_at; rec.n_cigar = h.n_cigar; rec.cg_at = ~0ull; rec.reserved = 0;
    bool placeholder = false;
    if (h.n_cigar) { const uint32_t op0 = bam_u32(b + cigar_at); placeholder = (op0 & 15u) == 4u && (op0 >> 4) == l_seq; }
    uint64_t tags_len = 0;
    for (uint64_t t_at = tags_at; t_at < end;) {
        BamTag t;
        if (const uint32_t reason = bam_next_tag(w, b, t_at, end, t)) return reason;
        if (placeholder && rec.cg_at == ~0ull && b[t_at] == 'C' && b[t_at + 1u] == 'G' && t.type == 'B' && t.sub == 'I') {
            rec.cg_at = t_at; rec.cigar_at = t.val_at; rec.n_cigar = t.count;
        } else {
            tags_len += 6u;                                          // "\tXX:T:"
            if (t.type == 'A') tags_len += 1u;
            else if (t.type == 'f') { const uint64_t slot = w.float_reserve(1u); if (w.lane == 0) w.float_put(slot, t.val_at); }
            else if (t.type == 'Z' || t.type == 'H') tags_len += t.len;
            else if (t.type == 'B') {
                tags_len += 1u;
                if (t.sub == 'f') {
                    tags_len += t.count;                             // the commas
                    const uint64_t slot = w.float_reserve(t.count);
                    for (uint64_t i = w.lane; i < t.count; i += W::LANES) w.float_put(slot + i, t.val_at + 4u * i);
                } else tags_len += bam_b_text<false>(w, b + t.val_at, t.sub, t.count, nullptr);
            } else tags_len += bam_sdec_len(bam_int_at(b + t.val_at, t.type));
        }
        t_at = t.next;
    }
    rec.cigar_len = rec.n_cigar ? bam_cigar_text<false>(w, b + rec.cigar_at, rec.n_cigar, nullptr) : 1u;
    rec.seq_at = bam_seq_at(h, R, rec.cigar_len);
    const uint64_t seq_len = l_seq ? l_seq : 1u, qual_len = (l_seq && b[qual_at] != 0xffu) ? l_seq : 1u;
    line_len = rec.seq_at + seq_len + 1u + qual_len + tags_len + 1u;
    n_slices = l_seq ? (uint32_t)((l_seq + BAM_SLICE_BASES - 1u) / BAM_SLICE_BASES) : 1u;
    return BAM_OK;
}

// a reference name, or `*`, at dst; its length
template <class W> NS_CSH uint64_t bam_w_ref(W &w, const BamRefs &R, int32_t id, uint8_t *dst) {
    if (id < 0) { if (w.lane == 0) dst[0] = '*'; return 1u; }
    const uint64_t n = R.off[id + 1] - R.off[id];
    bam_bulk<BAM_COPY>(w, R.names + R.off[id], n, dst);
    return n;
}
#define BAM_ROOM(n) do { if (cur + (uint64_t)(n) > line_len) return false; } while (0)
// ---- write: slice `slice` of the record into its line dst[0 .. line_len).  flt: the slots of the record's floats, in the order of the
// record.  false: the line is not what bam_measure measured (nothing was stored outside it) ----
template <class W> NS_CSH bool bam_write(W &w, const uint8_t *b, uint64_t at, uint64_t end, const BamRefs &R, const BamRec &rec, uint32_t slice,
                                         const uint8_t *flt, uint8_t *dst, uint64_t line_len) {
    BamHead h;
    bam_head(b + at + 4u, h);
    const uint64_t l_seq = (uint64_t)h.l_seq, name_at = at + 4u + BAM_FIXED, seq_at = name_at + h.l_name + 4ull * h.n_cigar,
                   qual_at = seq_at + (l_seq + 1u) / 2u, tags_at = qual_at + l_seq;
    const bool has_qual = l_seq && b[qual_at] != 0xffu;
    const uint64_t seq_len = l_seq ? l_seq : 1u, qual_len = has_qual ? l_seq : 1u;
    if (rec.seq_at != bam_seq_at(h, R, rec.cigar_len) || rec.seq_at + seq_len + 1u + qual_len + 1u > line_len) return false;
    const uint64_t lo = (uint64_t)slice * BAM_SLICE_BASES;
    if (lo < l_seq) {
        const uint64_t n = l_seq - lo < BAM_SLICE_BASES ? l_seq - lo : BAM_SLICE_BASES;
        bam_bulk<BAM_NIBBLE>(w, b + seq_at + lo / 2u, n, dst + rec.seq_at + lo);
        if (has_qual) bam_bulk<BAM_PLUS33>(w, b + qual_at + lo, n, dst + rec.seq_at + l_seq + 1u + lo);
    }
    if (slice) return true;
    const bool lane0 = w.lane == 0;
    uint64_t cur = 0;
    // QNAME FLAG RNAME POS MAPQ
    bam_bulk<BAM_COPY>(w, b + name_at, h.l_name - 1u, dst);
    cur = h.l_name - 1u;
    if (lane0) { dst[cur] = '\t'; bam_put_dec(dst + cur + 1u, h.flag, bam_dec_len(h.flag)); }
    cur += 1u + bam_dec_len(h.flag);
    if (lane0) dst[cur] = '\t';
    cur += 1u;
    cur += bam_w_ref(w, R, h.ref_id, dst + cur);
    if (lane0) { dst[cur] = '\t'; bam_put_sdec(dst + cur + 1u, (int64_t)h.pos + 1); }
    cur += 1u + bam_sdec_len((int64_t)h.pos + 1);
    if (lane0) { dst[cur] = '\t'; bam_put_dec(dst + cur + 1u, h.mapq, bam_dec_len(h.mapq)); dst[cur + 1u + bam_dec_len(h.mapq)] = '\t'; }
    cur += 2u + bam_dec_len(h.mapq);
    // CIGAR
    if (!rec.n_cigar) { if (lane0) dst[cur] = '*'; }
    else if (bam_cigar_text<true>(w, b + rec.cigar_at, rec.n_cigar, dst + cur) != rec.cigar_len) return false;
    cur += rec.cigar_len;
    // RNEXT PNEXT TLEN
    if (lane0) dst[cur] = '\t';
    cur += 1u;
    if (h.next_ref >= 0 && h.next_ref == h.ref_id) { if (lane0) dst[cur] = '='; cur += 1u; }
    else cur += bam_w_ref(w, R, h.next_ref, dst + cur);
    if (lane0) { dst[cur] = '\t'; bam_put_sdec(dst + cur + 1u, (int64_t)h.next_pos + 1); }
    cur += 1u + bam_sdec_len((int64_t)h.next_pos + 1);
    if (lane0) { dst[cur] = '\t'; bam_put_sdec(dst + cur + 1u, h.tlen); dst[cur + 1u + bam_sdec_len(h.tlen)] = '\t'; }
    cur += 2u + bam_sdec_len(h.tlen);
    if (cur != rec.seq_at) return false;
    // SEQ and QUAL: the slices' (checked above)
    if (lane0) {
        if (!l_seq) dst[cur] = '*';
        dst[cur + seq_len] = '\t';
        if (!has_qual) dst[cur + seq_len + 1u] = '*';
    }
    cur += seq_len + 1u + qual_len;
    // the tags
    for (uint64_t t_at = tags_at; t_at < end;) {
        BamTag t;
        if (bam_next_tag(w, b, t_at, end, t)) return false;
        if (t_at != rec.cg_at) {
            const uint8_t shown = (t.type == 'A' || t.type == 'f' || t.type == 'Z' || t.type == 'H' || t.type == 'B') ? t.type : (uint8_t)'i';
            const int64_t v = shown == 'i' ? bam_int_at(b + t.val_at, t.type) : 0;
            uint32_t fl = 0;                                         // f: the characters of its slot
            if (t.type == 'f') { fl = flt[BAM_FLOAT_SLOT - 1u]; if (fl > BAM_FLOAT_CHARS) fl = BAM_FLOAT_CHARS; }
            uint64_t body = 1u;                                      // A
            if (shown == 'i') body = bam_sdec_len(v);
            else if (t.type == 'f') body = fl;
            else if (t.type == 'Z' || t.type == 'H') body = t.len;
            else if (t.type == 'B') body = 1u + (t.sub == 'f' ? bam_bf_text<false>(w, flt, t.count, nullptr) : bam_b_text<false>(w, b + t.val_at, t.sub, t.count, nullptr));
            BAM_ROOM(6u + body);
            if (lane0) { dst[cur] = '\t'; dst[cur + 1u] = b[t_at]; dst[cur + 2u] = b[t_at + 1u]; dst[cur + 3u] = ':'; dst[cur + 4u] = shown; dst[cur + 5u] = ':'; }
            cur += 6u;
            if (shown == 'i') { if (lane0) bam_put_sdec(dst + cur, v); }
            else if (t.type == 'A') { if (lane0) dst[cur] = b[t.val_at]; }
            else if (t.type == 'f') { if (lane0) for (uint32_t k = 0; k < fl; ++k) dst[cur + k] = flt[k]; flt += BAM_FLOAT_SLOT; }
            else if (t.type == 'B') {
                if (lane0) dst[cur] = t.sub;
                if (t.sub == 'f') { bam_bf_text<true>(w, flt, t.count, dst + cur + 1u); flt += (uint64_t)t.count * BAM_FLOAT_SLOT; }
                else bam_b_text<true>(w, b + t.val_at, t.sub, t.count, dst + cur + 1u);
            } else bam_bulk<BAM_COPY>(w, b + t.val_at, t.len, dst + cur);
            cur += body;
        }
        t_at = t.next;
    }
    BAM_ROOM(1u);
    if (lane0) dst[cur] = '\n';
    return cur + 1u == line_len;
}
