// Test shim (CPU tests only): the engine's index of a SAM text (nanosim_amd/csrc/ns_sam_index.h — the code the k_sam_sep_*, k_sam_tags and
// k_sam_rows kernels run per chunk, per tab and per line) compiled for the HOST behind the signature of ns_sam_index, so that the masks,
// the two lists, the tag choice, the rows and the host module around the call are checked without a GPU.  The chunks are visited in the
// order of the text, span by span as the kernels cut it; the maximum — an atomic on the device — is a plain read and write, and the tabs
// offer in the order sam_host_set_order chooses: 0 text order, 1 reversed (the outcome must not depend on it).  The text is copied to a
// buffer of exactly its size: a read beyond it is an error under -fsanitize=address.  The bytes of the last chunk that lie behind the
// text are filled with '\n', '\t', '\r' and 0xff in turn, not with zeros: on the device they are whatever the allocation held before.
// Built by tests/test_sam_index.py with g++ into tests/_tmp/: as a shared library, and, with -DSAM_INDEX_MAIN, as a stand-alone program
// for -fsanitize=address,undefined that takes a SAM file and prints `n_records n_header n_odd n_cs n_md` and a checksum of the rows.
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../include/nanosim_amd.h"
#include "../nanosim_amd/csrc/ns_sam_index.h"

static_assert(sizeof(SamRow) == sizeof(ns_sam_row) && sizeof(SamSpan) == sizeof(ns_sam_span), "ns_sam_index.h mirrors the ABI structs");

struct HostOps {
    void max32(uint32_t *w, uint32_t v) const { if (v > *w) *w = v; }
};
static int g_order = 0;
static std::vector<SamRow> g_rows;
static std::vector<SamSpan> g_header;

extern "C" void sam_host_set_order(int order) { g_order = order; }
extern "C" uint64_t sam_host_span(void) { return SAM_SPAN; }

extern "C" int sam_host_index(void *, const uint8_t *text_in, uint64_t nbytes, ns_sam_index_result *out) {
    if (!out) return -1;
    g_rows.clear(); g_header.clear();
    out->rows = nullptr; out->header = nullptr;
    out->n_records = out->n_header = out->n_odd = out->n_cs = out->n_md = 0; out->ms_kernel = 0;
    if (nbytes && !text_in) return -1;
    if (!nbytes) return 0;
    const std::vector<uint8_t> exact(text_in, text_in + nbytes);
    const uint8_t *text = exact.data();
    // the separators: chunk by chunk in the order of the text (a span's chunks (load, lane) are consecutive)
    std::vector<uint64_t> line_start{0}, line_rank{0}, tab_pos;
    std::vector<uint32_t> tab_line;
    static const uint8_t dirty[4] = {'\n', '\t', '\r', 0xff};
    static uint32_t g_turn = 0;
    uint32_t turn = g_turn++;                                      // (every call begins with another of the four)
    for (uint64_t at = 0; at < nbytes; at += SAM_CHUNK) {
        const uint32_t valid = nbytes - at >= SAM_CHUNK ? SAM_CHUNK : (uint32_t)(nbytes - at);
        uint8_t bytes[SAM_CHUNK];
        uint32_t w[4];
        memcpy(bytes, text + at, valid);
        for (uint32_t k = valid; k < SAM_CHUNK; ++k) bytes[k] = dirty[turn++ & 3u];     // what the device may find there: only sam_chunk's `keep` hides it
        memcpy(w, bytes, sizeof w);
        const SamChunk c = sam_chunk(w, valid);
        out->n_odd += (uint64_t)__builtin_popcount(c.odd);
        const uint64_t nl_at = line_start.size() - 1u, tab_at = tab_pos.size();
        for (uint32_t k = 0; k < SAM_CHUNK; ++k) {
            if (c.tab >> k & 1u) { tab_pos.push_back(at + k); tab_line.push_back((uint32_t)(nl_at + (uint32_t)__builtin_popcount(sam_below(c.nl, k)))); }
            if (c.nl >> k & 1u) { line_start.push_back(at + k + 1u); line_rank.push_back(tab_at + (uint32_t)__builtin_popcount(sam_below(c.tab, k))); }
        }
    }
    const uint64_t n_nl = line_start.size() - 1u, n_tabs = tab_pos.size();
    const uint64_t n_lines = n_nl + (text[nbytes - 1u] == '\n' ? 0u : 1u);
    if (n_lines > n_nl) { line_start.push_back(nbytes + 1u); line_rank.push_back(n_tabs); }
    if (n_lines >= (1ull << 32)) return -1;
    const SamLists L{line_start.data(), line_rank.data(), tab_pos.data(), n_lines, nbytes};
    std::vector<uint32_t> slots(n_lines * SAM_TAGS, 0u);
    HostOps ops;
    for (uint64_t i = 0; i < n_tabs; ++i) {
        const uint64_t tab = g_order == 1 ? n_tabs - 1u - i : i;
        sam_tag_offer(text, L, tab, tab_line[tab], slots.data(), ops);
    }
    for (uint64_t l = 0; l < n_lines; ++l) {
        SamRow R; SamSpan H;
        memset(&R, 0, sizeof R);
        const int what = sam_row(text, L, l, slots.data(), R, H);
        if (what == SAM_LINE_TOO_LONG) return -1;
        if (what == SAM_LINE_HEADER) { g_header.push_back(H); continue; }
        g_rows.push_back(R);
        if (R.bits & SAM_HAS_CS) out->n_cs += 1;
        if (R.bits & SAM_HAS_MD) out->n_md += 1;
    }
    out->n_records = g_rows.size(); out->n_header = g_header.size();
    out->rows = reinterpret_cast<const ns_sam_row *>(g_rows.data());
    out->header = reinterpret_cast<const ns_sam_span *>(g_header.data());
    return 0;
}

#ifdef SAM_INDEX_MAIN
#include <stdio.h>
int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint8_t> text;
    uint8_t buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) text.insert(text.end(), buf, buf + n);
    fclose(f);
    unsigned long long sums[2] = {0, 0};
    for (int order = 0; order < 2; ++order) {
        ns_sam_index_result out;
        memset(&out, 0, sizeof out);
        sam_host_set_order(order);
        if (sam_host_index(nullptr, text.data(), text.size(), &out)) return 3;
        unsigned long long sum = 0;
        for (uint64_t k = 0; k < out.n_records; ++k) {
            const ns_sam_row &r = out.rows[k];
            sum = (((sum * 31u + r.begin) * 31u + r.end) * 31u + r.n_fields) * 31u + r.bits;
            for (int j = 0; j < 11; ++j) sum = sum * 31u + r.field_end[j];
            sum = ((sum * 31u + r.flag) * 31u + r.pos) * 31u + r.nm;
            for (int j = 0; j < 4; ++j) sum = (sum * 31u + r.tag_at[j]) * 31u + r.tag_len[j];
        }
        for (uint64_t k = 0; k < out.n_header; ++k) sum = (sum * 31u + out.header[k].begin) * 31u + out.header[k].end;
        sums[order] = sum;
        if (order == 0)
            printf("%llu %llu %llu %llu %llu\n", (unsigned long long)out.n_records, (unsigned long long)out.n_header, (unsigned long long)out.n_odd,
                   (unsigned long long)out.n_cs, (unsigned long long)out.n_md);
    }
    if (sums[0] != sums[1]) return 4;
    printf("%llu\n", sums[0]);
    return 0;
}
#endif
