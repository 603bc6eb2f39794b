// Test shim (CPU tests only): the engine's BAM-to-SAM walks (nanosim_amd/csrc/ns_bam.h — the code the k_bam_* kernels run per wavefront)
// compiled for the HOST behind the signature of ns_bam_to_sam, with a wavefront of ONE lane: the prefix sums, the search for a NUL and
// the striding of the bulk fields are the same code with 1 in the place of 64.  The bytes are copied to a buffer of exactly the size
// of the whole records and every line is written into a buffer of exactly its measured size: a read or a write beyond either is an
// error under -fsanitize=address.
// Built by tests/test_bam.py with g++ into tests/_tmp/: as a shared library, and, with -DBAM_HOST_MAIN, as a stand-alone program for
// -fsanitize=address,undefined: `bam_host <file of inflated records> <final> [reference name ...]` prints
// `n_records n_text consumed first_bad first_bad_offset bad_reason` and a checksum of the text and the offsets.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "../include/nanosim_amd.h"
#include "../nanosim_amd/csrc/ns_bam.h"

struct BamWaveHost {
    static constexpr uint32_t LANES = 1u;
    uint32_t lane;
    std::vector<uint64_t> *flt_at;
    uint32_t scan(uint32_t v, uint32_t &total) const { total = v; return 0u; }
    uint32_t first(bool pred) const { return pred ? 0u : 1u; }
    uint32_t bcast(uint32_t v, uint32_t) const { return v; }
    uint64_t float_reserve(uint32_t n) const { const uint64_t at = flt_at->size(); flt_at->resize(at + n); return at; }
    void float_put(uint64_t slot, uint64_t where) const { (*flt_at)[slot] = where; }
};

static std::vector<uint8_t> g_text;
static std::vector<uint64_t> g_line_off;

extern "C" uint32_t bam_host_constant(int which) {
    const uint32_t v[] = {BAM_ROUND_OPS, BAM_LANE_BYTES, BAM_SLICE_BASES, BAM_STRLEN_BYTES, BAM_FLOAT_SLOT, BAM_FLOAT_CHARS};
    return which >= 0 && which < 6 ? v[which] : 0u;
}

extern "C" int bam_host_to_sam(void *, const uint8_t *bytes_in, uint64_t nbytes, int final, const uint8_t *ref_names, const uint64_t *ref_off, uint32_t n_ref,
                               ns_bam_result *out) {
    if (!out) return -1;
    g_text.clear(); g_line_off.clear();
    out->text = nullptr; out->line_off = nullptr; out->n_records = out->n_text = out->consumed = 0; out->first_bad = ~0ull; out->first_bad_offset = ~0ull;
    out->bad_reason = NS_BAM_OK; out->reserved = 0; out->ms_kernel = 0;
    if ((nbytes && !bytes_in) || (n_ref && !ref_off)) return -1;
    if (n_ref) {
        if (ref_off[0]) return -1;
        for (uint32_t i = 0; i < n_ref; ++i) if (ref_off[i] > ref_off[i + 1]) return -1;
        if (ref_off[n_ref] && !ref_names) return -1;
    }
    std::vector<uint64_t> off;
    uint64_t at = 0, host_bad = ~0ull;
    uint32_t host_reason = NS_BAM_OK;
    while (nbytes - at >= 4u) {
        int32_t bs;
        memcpy(&bs, bytes_in + at, 4);
        if (bs < 0) { host_bad = off.size(); host_reason = NS_BAM_BAD_BLOCK_SIZE; break; }
        if ((uint64_t)bs > nbytes - at - 4u) break;
        off.push_back(at);
        at += 4ull + (uint64_t)bs;
    }
    if (host_bad == ~0ull && final && at < nbytes) { host_bad = off.size(); host_reason = NS_BAM_BAD_TRUNCATED; }
    off.push_back(at);
    const uint32_t n = (uint32_t)(off.size() - 1u);
    const std::vector<uint8_t> exact(bytes_in, bytes_in + at), exact_names(ref_names, ref_names + (n_ref ? ref_off[n_ref] : 0));
    const uint8_t *b = exact.data();
    const BamRefs R{exact_names.data(), ref_off, n_ref};
    std::vector<uint64_t> flt_at;
    BamWaveHost w{0u, &flt_at};
    std::vector<BamRec> rec(n);
    std::vector<uint64_t> len(n);
    std::vector<uint32_t> slices(n), flt_first(n + 1u, 0u);
    for (uint32_t r = 0; r < n; ++r) {
        flt_first[r] = (uint32_t)flt_at.size();
        if (const uint32_t reason = bam_measure(w, b, off[r], off[r + 1u], R, rec[r], len[r], slices[r])) {
            out->first_bad = r; out->first_bad_offset = off[r]; out->bad_reason = reason;
            return 0;
        }
    }
    flt_first[n] = (uint32_t)flt_at.size();
    if (host_bad != ~0ull) { out->first_bad = host_bad; out->first_bad_offset = at; out->bad_reason = host_reason; return 0; }
    if (!std::is_sorted(flt_at.begin(), flt_at.end())) return -2;
    std::vector<uint8_t> slots(flt_at.size() * BAM_FLOAT_SLOT + 1u, 0);
    for (size_t k = 0; k < flt_at.size(); ++k) {
        float f;
        memcpy(&f, b + flt_at[k], 4);
        char buf[32];
        int l = snprintf(buf, sizeof buf, "%g", (double)f);
        if (l < 0 || l > (int)BAM_FLOAT_CHARS) return -3;
        memcpy(&slots[k * BAM_FLOAT_SLOT], buf, (size_t)l);
        slots[k * BAM_FLOAT_SLOT + BAM_FLOAT_SLOT - 1u] = (uint8_t)l;
    }
    g_line_off.push_back(0);
    for (uint32_t r = 0; r < n; ++r) {
        uint64_t ll = len[r];
        for (uint32_t k = flt_first[r]; k < flt_first[r + 1u]; ++k) ll += slots[k * BAM_FLOAT_SLOT + BAM_FLOAT_SLOT - 1u];
        // a line of exactly its size, at every alignment the device's text can give it: the pieces of bam_bulk depend on it
        std::vector<uint8_t> line(ll + 2u * BAM_LANE_BYTES, 0xee);
        uint8_t *base = line.data();
        base += (BAM_LANE_BYTES - ((uintptr_t)base & (BAM_LANE_BYTES - 1u))) & (BAM_LANE_BYTES - 1u);
        uint8_t *dst = base + (g_text.size() & (BAM_LANE_BYTES - 1u));
        for (uint32_t k = 0; k < slices[r]; ++k)
            if (!bam_write(w, b, off[r], off[r + 1u], R, rec[r], k, slots.data() + (size_t)flt_first[r] * BAM_FLOAT_SLOT, dst, ll)) return -4;
        for (uint8_t *p = line.data(); p < dst; ++p) if (*p != 0xee) return -5;
        for (uint8_t *p = dst + ll; p < line.data() + line.size(); ++p) if (*p != 0xee) return -5;
        g_text.insert(g_text.end(), dst, dst + ll);
        g_line_off.push_back(g_text.size());
    }
    out->text = g_text.data(); out->line_off = g_line_off.data();
    out->n_records = n; out->n_text = g_text.size(); out->consumed = at;
    return 0;
}

#ifdef BAM_HOST_MAIN
#include <stdlib.h>
int main(int argc, char **argv) {
    if (argc < 3) return 2;
    std::vector<uint8_t> bytes, names;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint8_t buf[1 << 16];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) bytes.insert(bytes.end(), buf, buf + got);
    fclose(f);
    std::vector<uint64_t> off{0};
    for (int i = 3; i < argc; ++i) { names.insert(names.end(), argv[i], argv[i] + strlen(argv[i])); off.push_back(names.size()); }
    ns_bam_result out;
    const std::vector<uint8_t> exact(bytes);                                         // (exactly its size: the hop over the chain is checked too)
    const int rc = bam_host_to_sam(nullptr, exact.data(), exact.size(), atoi(argv[2]), names.data(), off.data(), (uint32_t)(off.size() - 1u), &out);
    if (rc) return 3;
    unsigned long long sum = 0;
    for (uint64_t i = 0; i < out.n_text; ++i) sum = sum * 31u + out.text[i];
    for (uint64_t i = 0; i <= out.n_records && out.line_off; ++i) sum = sum * 31u + out.line_off[i];
    printf("%llu %llu %llu %lld %lld %u\n%llu\n", (unsigned long long)out.n_records, (unsigned long long)out.n_text, (unsigned long long)out.consumed,
           (long long)out.first_bad, (long long)out.first_bad_offset, out.bad_reason, sum);
    return 0;
}
#endif
