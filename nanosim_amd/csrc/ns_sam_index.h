// ns_sam_index.h — training side, the index of a SAM text ("SAM text: one indexed pass and the CLI"): where the lines, the
// fields and the four tags the readers look for stand in the bytes of the file, so that no reader splits a line again.  The rules are
// those of characterize.sam_text (_sam_records, sam_tag) and of chimeric_records' tag loop:
//   lines   a line begins at byte 0 or behind a '\n' and ends in front of the next '\n' or at the end of the text.  A line whose first
//           byte is `@` is a header line, wherever it stands.  An empty line is a record of one empty field.
//   fields  what split("\t") gives: every tab separates, empty fields count, n_fields = tabs + 1.
//   tags    among the fields 11 onwards, the prefixes cs:Z: MD:Z: NM:i: SA:Z:; of several fields with one prefix the LAST wins.  The
//           value runs from behind the five prefix bytes to the field's end (it may be empty); a field of fewer than five bytes is no tag.
//   numbers FLAG (field 1), POS (field 3) and the NM:i: value are PLAIN when they are 1-10 decimal digits with a value below 2^32.  What
//           is not plain — a sign, a blank, an underscore, an overflow, an empty field — only sets the row's bit for that number:
//           Python's int() takes some of these, and the host decides.
//   odd     the bytes that are '\r' or >= 0x80 are counted, nothing more: text mode (universal newlines, UTF-8) is not restated.
// How it is found.  The separators carry all the structure and are rare (a dozen tabs in tens of kilobytes of SEQ and QUAL), so nothing
// walks a line.  The text is cut into spans of SAM_SPAN bytes and a span into chunks of SAM_CHUNK; a chunk gives two bit masks
// (sam_chunk: its '\n' and its '\t' bytes).  From the masks come two ascending lists — the line starts, each with its TAB RANK (the
// number of tabs in front of it), and the tab positions, each with its line — and then
//   field k of line l   is bounded by the tabs rank[l] + k - 1 and rank[l] + k where these are below rank[l + 1]   (sam_field)
//   n_fields            = rank[l + 1] - rank[l] + 1
//   tags                every tab whose field index is >= 11 compares the bytes behind it with the prefixes and offers its field index
//                       to the line's slot for that tag by a maximum (sam_tag_offer): the last field wins in any order of arrival
//   rows                one row per line from the lists and the settled slots (sam_row)
// The lists have one entry more than there are lines: line_start[n_lines] is one past where a further line would begin (nbytes + 1
// behind a last line without '\n'), so that the end of line l is always line_start[l + 1] - 1, and line_rank[n_lines] the number of tabs.
// The code below compiles for the device (k_sam_sep_*, k_sam_tags, k_sam_rows in ns_train.h) and, unchanged, for the host
// (tests/sam_index_host.cpp), where the maximum is a plain read and write (the `Ops` argument).
#pragma once
#include <stdint.h>
#include "ns_cs_hist.h"

#define SAM_SPAN 16384u                               // the bytes of the text one workgroup of the separator kernels looks at
#define SAM_CHUNK 16u                                 // ... one lane with one load
#define SAM_LOADS 4u                                  // ... in so many loads of 256 lanes: load i of a span covers its bytes 4096 i .. 4096 i + 4095
#define SAM_TAGS 4u
#define SAM_TAG_FIELD 11u                             // the first field that may be a tag
enum { SAM_TAG_CS = 0, SAM_TAG_MD = 1, SAM_TAG_NM = 2, SAM_TAG_SA = 3 };
enum { SAM_FLAG_ODD = 1u, SAM_POS_ODD = 2u, SAM_NM_ODD = 4u,                   // SamRow.bits: the number is not plain (NM: of a row that has the tag)
       SAM_HAS_CS = 16u, SAM_HAS_MD = 32u, SAM_HAS_NM = 64u, SAM_HAS_SA = 128u };  // ... SAM_HAS_CS << tag: the row has the tag
enum { SAM_LINE_RECORD = 0, SAM_LINE_HEADER = 1, SAM_LINE_TOO_LONG = 2 };     // what sam_row says of a line

// one record (= ns_sam_row of include/nanosim_amd.h).  Everything but begin and end is relative to begin.
struct SamRow {
    uint64_t begin, end;                              // the line in the text; end: its '\n' or the end of the text
    uint32_t n_fields, bits;
    uint32_t field_end[11];                           // where fields 0 .. 10 end (field k + 1 begins one behind); the line's length for a field it has not
    uint32_t flag, pos, nm;                           // 0 where not plain or absent
    uint32_t tag_at[SAM_TAGS], tag_len[SAM_TAGS];     // the values of cs, MD, NM, SA (0, 0 without the tag)
};
struct SamSpan { uint64_t begin, end; };              // a header line (= ns_sam_span)

// the bytes of a 32-bit word that equal c / that are >= 0x80, as 4 bits (bit k: byte k, in memory order)
NS_CSH uint32_t sam_gather4(uint32_t z) { return (((z >> 7) & 0x01010101u) * 0x00204081u >> 21) & 0xfu; }
NS_CSH uint32_t sam_eq4(uint32_t w, uint32_t c) {
    const uint32_t x = w ^ (c * 0x01010101u);
    return sam_gather4(~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu));          // (0x80 in exactly the bytes of x that are 0)
}
// a chunk: 16 bytes as four words, of which the first `valid` belong to the text -> bit k of a mask: byte k is '\n' / '\t' / odd
struct SamChunk { uint32_t nl, tab, odd; };
NS_CSH SamChunk sam_chunk(const uint32_t w[4], uint32_t valid) {
    SamChunk c = {0u, 0u, 0u};
    for (uint32_t k = 0; k < 4u; ++k) {
        c.nl |= sam_eq4(w[k], '\n') << (4u * k);
        c.tab |= sam_eq4(w[k], '\t') << (4u * k);
        c.odd |= (sam_eq4(w[k], '\r') | sam_gather4(w[k] & 0x80808080u)) << (4u * k);
    }
    const uint32_t keep = valid >= SAM_CHUNK ? 0xffffu : (1u << valid) - 1u;
    c.nl &= keep; c.tab &= keep; c.odd &= keep;
    return c;
}
NS_CSH uint32_t sam_below(uint32_t mask, uint32_t k) { return mask & ((1u << k) - 1u); }             // the bits of a mask in front of bit k
template <class S> NS_CSH bool sam_is_header(S &t, uint64_t nbytes, uint64_t begin) { return begin < nbytes && t[begin] == '@'; }

// the two lists (the header comment says what the entries behind the last line are)
struct SamLists {
    const uint64_t *line_start, *line_rank;           // n_lines + 1 each
    const uint64_t *tab_pos;                          // line_rank[n_lines]
    uint64_t n_lines, nbytes;
};
// field k of line l (k < its n_fields): [b, e) in the text
NS_CSH void sam_field(const SamLists &L, uint64_t l, uint64_t k, uint64_t &b, uint64_t &e) {
    const uint64_t r0 = L.line_rank[l], r1 = L.line_rank[l + 1u];
    b = k ? L.tab_pos[r0 + k - 1u] + 1u : L.line_start[l];
    e = r0 + k < r1 ? L.tab_pos[r0 + k] : L.line_start[l + 1u] - 1u;
}
// the tag whose prefix the field [b, e) begins with, -1 without
template <class S> NS_CSH int sam_tag_of(S &t, uint64_t b, uint64_t e) {
    if (e - b < 5u) return -1;
    const uint8_t c0 = t[b], c1 = t[b + 1u], c2 = t[b + 2u], c3 = t[b + 3u], c4 = t[b + 4u];
    if (c2 != ':' || c4 != ':') return -1;
    if (c0 == 'c' && c1 == 's' && c3 == 'Z') return SAM_TAG_CS;
    if (c0 == 'M' && c1 == 'D' && c3 == 'Z') return SAM_TAG_MD;
    if (c0 == 'N' && c1 == 'M' && c3 == 'i') return SAM_TAG_NM;
    if (c0 == 'S' && c1 == 'A' && c3 == 'Z') return SAM_TAG_SA;
    return -1;
}
// tab number `tab` of the text, which stands in line l: the field behind it offers its index to the line's slot of its tag.
// slots: SAM_TAGS words per line, preset to 0 (no field: a tag's index is >= 11).  Ops::max32(word, value): word = max(word, value)
template <class S, class Ops> NS_CSH void sam_tag_offer(S &t, const SamLists &L, uint64_t tab, uint64_t l, uint32_t *slots, Ops &ops) {
    const uint64_t k = tab - L.line_rank[l] + 1u;
    if (k < SAM_TAG_FIELD || k > 0xffffffffull) return;                 // (beyond 32 bits: the line is too long, and sam_row says so)
    uint64_t b, e;
    sam_field(L, l, k, b, e);
    const int tag = sam_tag_of(t, b, e);
    if (tag >= 0) ops.max32(slots + SAM_TAGS * l + (uint32_t)tag, (uint32_t)k);
}
// the plain number in [b, e); false: not plain (v = 0)
template <class S> NS_CSH bool sam_number(S &t, uint64_t b, uint64_t e, uint32_t &v) {
    v = 0;
    if (e == b || e - b > 10u) return false;
    uint64_t x = 0;
    for (uint64_t i = b; i < e; ++i) {
        const uint8_t c = t[i];
        if (c < '0' || c > '9') return false;
        x = x * 10u + (uint64_t)(c - '0');
    }
    if (x > 0xffffffffull) return false;
    v = (uint32_t)x;
    return true;
}
// line l, after every tab has offered: a record (R is its row), a header line (H is its span) or a line of 2^32 bytes or more
template <class S> NS_CSH int sam_row(S &t, const SamLists &L, uint64_t l, const uint32_t *slots, SamRow &R, SamSpan &H) {
    const uint64_t begin = L.line_start[l], end = L.line_start[l + 1u] - 1u, r0 = L.line_rank[l], tabs = L.line_rank[l + 1u] - r0;
    if (end - begin > 0xffffffffull) return SAM_LINE_TOO_LONG;
    if (sam_is_header(t, end, begin)) { H.begin = begin; H.end = end; return SAM_LINE_HEADER; }
    R.begin = begin; R.end = end;
    R.n_fields = tabs >= 0xffffffffull ? 0xffffffffu : (uint32_t)tabs + 1u;
    R.bits = 0;
    for (uint32_t k = 0; k < 11u; ++k) R.field_end[k] = (uint32_t)((k < tabs ? L.tab_pos[r0 + k] : end) - begin);
    if (tabs < 1u || !sam_number(t, begin + R.field_end[0] + 1u, begin + R.field_end[1], R.flag)) { R.flag = 0; R.bits |= SAM_FLAG_ODD; }
    if (tabs < 3u || !sam_number(t, begin + R.field_end[2] + 1u, begin + R.field_end[3], R.pos)) { R.pos = 0; R.bits |= SAM_POS_ODD; }
    R.nm = 0;
    for (uint32_t g = 0; g < SAM_TAGS; ++g) {
        const uint32_t k = slots[SAM_TAGS * l + g];
        R.tag_at[g] = R.tag_len[g] = 0;
        if (!k) continue;
        uint64_t b, e;
        sam_field(L, l, k, b, e);
        R.tag_at[g] = (uint32_t)(b + 5u - begin); R.tag_len[g] = (uint32_t)(e - b - 5u);
        R.bits |= SAM_HAS_CS << g;
        if (g == SAM_TAG_NM && !sam_number(t, b + 5u, e, R.nm)) R.bits |= SAM_NM_ODD;
    }
    return SAM_LINE_RECORD;
}
