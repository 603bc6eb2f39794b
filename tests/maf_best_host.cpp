// Test shim (CPU tests only): the engine's best-hit choice over a MAF file (nanosim_amd/csrc/ns_maf_best.h — the code the k_maf_* kernels
// run per thread) compiled for the HOST behind the signature of ns_maf_besthit, so that the line test, the field parser, the table and
// the host module around the call are checked against the reference's fixture without a GPU.  The two table operations — atomics on the
// device — are a plain read-compare-write and a plain maximum here, and the pairs visit the table one after the other, in the order
// maf_host_set_order chooses: 0 file order, 1 reversed, 2 a fixed shuffle (the outcome must not depend on it).  The text is copied to
// a buffer of exactly its size: a read beyond it is an error under -fsanitize=address.
// Built by tests/test_besthit.py with g++ into tests/_tmp/: as a shared library, and, with -DMAF_BEST_MAIN, as a stand-alone program for
// -fsanitize=address,undefined that takes a MAF file and, optionally, a file of names (one per line) and prints
// `n_lines n_pairs n_kept pos_strand first_bad_line`, a checksum of the per-kept-pair arrays and the found bytes.
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "../include/nanosim_amd.h"
#include "../nanosim_amd/csrc/ns_maf_best.h"

static_assert(sizeof(MafOutLines) == sizeof(ns_maf_best_lines) && sizeof(MafOutRecord) == sizeof(ns_maf_best_record) &&
              sizeof(MafOutFigures) == sizeof(ns_maf_best_figures), "ns_maf_best.h mirrors the ABI structs");

struct HostOps {
    uint32_t cas(uint32_t *w, uint32_t expected, uint32_t desired) const { const uint32_t old = *w; if (old == expected) *w = desired; return old; }
    void max64(unsigned long long *w, unsigned long long v) const { if (v > *w) *w = v; }
};
static int g_order = 0;
static std::vector<MafOutLines> g_lines;
static std::vector<MafOutRecord> g_records;
static std::vector<MafOutFigures> g_figures;

extern "C" void maf_host_set_order(int order) { g_order = order; }
extern "C" uint64_t maf_host_line_span(void) { return MAF_LINE_SPAN; }

extern "C" int maf_host_besthit(void *, const uint8_t *text_in, uint64_t nbytes, const uint8_t *names_in, const uint64_t *names_off, uint32_t n_names,
                                ns_maf_best_result *out) {
    if (!out) return -1;
    g_lines.clear(); g_records.clear(); g_figures.clear();
    out->lines = nullptr; out->records = nullptr; out->figures = nullptr;
    out->n_lines = out->n_pairs = out->n_kept = out->pos_strand = 0; out->first_bad_line = 0; out->first_bad_offset = ~0ull; out->ms_kernel = 0;
    if ((nbytes && !text_in) || (n_names && (!names_off || !out->found))) return -1;
    if (n_names) {
        if (names_off[0]) return -1;
        for (uint32_t i = 0; i < n_names; ++i) if (names_off[i] > names_off[i + 1]) return -1;
        memset(out->found, 0, n_names);
    }
    if (!nbytes) return 0;
    const std::vector<uint8_t> exact(text_in, text_in + nbytes), exact_names(names_in, names_in + (n_names ? names_off[n_names] : 0));
    const uint8_t *text = exact.data(), *text2 = exact.data(), *names = exact_names.data();
    std::vector<uint64_t> starts;
    for (uint64_t i = 0; i < nbytes; ++i) if (maf_is_start(text, nbytes, i)) starts.push_back(i);
    const uint64_t n_lines = starts.size();
    out->n_lines = out->first_bad_line = n_lines;
    if (n_lines & 1u) return -1;
    if (n_lines >= (1ull << 32)) return -1;
    const uint32_t n_pairs = (uint32_t)(n_lines / 2u);
    out->n_pairs = n_pairs;
    std::vector<MafLine> lines(n_lines);
    for (uint64_t l = 0; l < n_lines; ++l)
        if (!maf_parse_line(text, nbytes, starts[l], lines[l]) && out->first_bad_line == n_lines) { out->first_bad_line = l; out->first_bad_offset = starts[l]; }
    if (out->first_bad_line != n_lines) return 0;
    uint64_t slots = 2;
    while (slots < 2ull * n_pairs) slots <<= 1;
    std::vector<uint32_t> owner(slots, MAF_EMPTY), slot_of(n_pairs), order(n_pairs);
    std::vector<unsigned long long> key(slots, 0ull);
    const MafTable T{owner.data(), key.data(), slots};
    for (uint32_t p = 0; p < n_pairs; ++p) order[p] = p;
    if (g_order == 1) std::reverse(order.begin(), order.end());
    if (g_order == 2) {
        uint64_t x = 88172645463325252ull;                                         // xorshift64: a fixed shuffle
        for (uint32_t i = n_pairs; i > 1; --i) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; std::swap(order[i - 1], order[x % i]); }
    }
    HostOps ops;
    for (uint32_t p : order) {
        const MafLine &Q = lines[2ull * p + 1u];
        const uint64_t slot = maf_claim(text, text2, lines.data(), T, p, Q, ops);
        if (slot >= slots) return -2;
        maf_offer(T, slot, p, Q.size, ops);
        slot_of[p] = (uint32_t)slot;
    }
    for (uint32_t p = 0; p < n_pairs; ++p) {
        if (!maf_kept(T, slot_of[p], p)) continue;
        const MafLine &R = lines[2ull * p], &Q = lines[2ull * p + 1u];
        if (maf_same_bytes(text, R.strand_at, R.strand_len, text2, Q.strand_at, Q.strand_len)) out->pos_strand += 1;
        MafOutLines ol; MafOutRecord orc; MafOutFigures of;
        maf_emit(nbytes, starts[2ull * p], R, starts[2ull * p + 1u], Q, ol, orc, of);
        g_lines.push_back(ol); g_records.push_back(orc); g_figures.push_back(of);
    }
    for (uint32_t i = 0; i < n_names; ++i) {
        const uint64_t n = names_off[i + 1] - names_off[i];
        out->found[i] = n <= 0xffffffffull && maf_find(text, lines.data(), T, names, names_off[i], (uint32_t)n) ? 1 : 0;
    }
    out->n_kept = g_lines.size();
    out->lines = reinterpret_cast<const ns_maf_best_lines *>(g_lines.data());
    out->records = reinterpret_cast<const ns_maf_best_record *>(g_records.data());
    out->figures = reinterpret_cast<const ns_maf_best_figures *>(g_figures.data());
    return 0;
}

#ifdef MAF_BEST_MAIN
#include <stdio.h>
#include <string>
static bool slurp(const char *path, std::vector<uint8_t> &to) {
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    uint8_t buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) to.insert(to.end(), buf, buf + n);
    fclose(f);
    return true;
}
int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::vector<uint8_t> text, list, names;
    if (!slurp(argv[1], text)) return 2;
    std::vector<uint64_t> off{0};
    if (argc > 2) {
        if (!slurp(argv[2], list)) return 2;
        for (size_t i = 0, b = 0; i <= list.size(); ++i)
            if (i == list.size() || list[i] == '\n') { if (i > b) { names.insert(names.end(), list.begin() + b, list.begin() + i); off.push_back(names.size()); } b = i + 1; }
    }
    const uint32_t n_names = (uint32_t)(off.size() - 1);
    std::vector<uint8_t> found(n_names);
    unsigned long long sums[3] = {0, 0, 0};
    for (int order = 0; order < 3; ++order) {
        ns_maf_best_result out;
        memset(&out, 0, sizeof out);
        out.found = found.data();
        maf_host_set_order(order);
        const int rc = maf_host_besthit(nullptr, text.data(), text.size(), names.data(), off.data(), n_names, &out);
        if (rc && !(out.n_lines & 1u)) return 3;
        unsigned long long sum = 0;
        for (uint64_t k = 0; k < out.n_kept; ++k)
            sum = ((sum * 31u + out.lines[k].ref_begin) * 31u + out.lines[k].qry_end) * 31u + out.records[k].ref_start + (unsigned long long)out.figures[k].ht;
        for (uint8_t f : found) sum = sum * 31u + f;
        sums[order] = sum;
        if (order == 0)
            printf("%llu %llu %llu %llu %llu\n", (unsigned long long)out.n_lines, (unsigned long long)out.n_pairs, (unsigned long long)out.n_kept,
                   (unsigned long long)out.pos_strand, (unsigned long long)out.first_bad_line);
    }
    if (sums[0] != sums[1] || sums[0] != sums[2]) return 4;
    printf("%llu\n", sums[0]);
    return 0;
}
#endif
