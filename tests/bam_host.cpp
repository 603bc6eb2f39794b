// Test shim (CPU tests only): the engine's BAM-to-SAM walks (nanosim_amd/csrc/ns_bam.h — the code the k_bam_* kernels run per wavefront)
// compiled for the HOST behind the signature of ns_bam_to_sam, with a wavefront of ONE lane: the prefix sums, the search for a NUL and
// the striding of the bulk fields are the same code with 1 in the place of 64.  The bytes are copied to a buffer of exactly the size
// of the whole records and every line is written into a buffer of exactly its measured size: a read or a write beyond either is an
// error under -fsanitize=address.
// With -DBAM_HOST_LANES=64 the wavefront has 64 lanes in lock step (tests/wave64_host.h; tests/test_bam_wave64.py): the guards of the
// rounds, the striding of the bulk fields and the search for a NUL are then what the GPU runs.
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

#ifndef BAM_HOST_LANES
#define BAM_HOST_LANES 1
#endif
#if BAM_HOST_LANES == 64
// -DBAM_HOST_LANES=64: the same walks on the lock-step wavefront of tests/wave64_host.h, 64 host threads (-pthread), behind the same
// signatures.  float_reserve: the lanes meet, lane 0 makes room in the list (no lane is still putting into it), its place comes back
// to all of them through a second meeting (both order memory, as the device's atomic add on a list that never moves need not).  Every lane keeps what the walk returns to it; the lanes have to agree.
#include "wave64_host.h"
struct BamWaveHost : Wave64Lane {
    std::vector<uint64_t> *flt_at;
    BamWaveHost(Wave64 *wv, uint32_t l, std::vector<uint64_t> *f) : Wave64Lane{wv, l}, flt_at(f) {}
    uint64_t float_reserve(uint32_t n) const {
        uint64_t s[LANES], at = 0;
        wave->meet(lane, Wave64::RESERVE_IN, n, s);
        if (lane == 0) { at = flt_at->size(); flt_at->resize(at + n); }
        wave->meet(lane, Wave64::RESERVE_OUT, at, s);
        return s[0];
    }
    void float_put(uint64_t slot, uint64_t where) const { (*flt_at)[slot] = where; }
};
static Wave64 g_wave;
template <class F> static bool on_wave(std::vector<uint64_t> *flt_at, F f) {
    return g_wave.run([&](uint32_t lane) { BamWaveHost w(&g_wave, lane, flt_at); f(w); });
}
#elif BAM_HOST_LANES == 1
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
template <class F> static bool on_wave(std::vector<uint64_t> *flt_at, F f) { BamWaveHost w{0u, flt_at}; f(w); return true; }
#else
#error "BAM_HOST_LANES is 1 or 64"
#endif

// bam_measure and bam_write on the wave.  0; -6: the wave stopped (tests/wave64_host.h); -7: the lanes disagree on what the walk returns
struct BamMeasured { uint32_t reason, n_slices; BamRec rec; uint64_t line_len; };
static int measure_on_wave(std::vector<uint64_t> *flt_at, const uint8_t *b, uint64_t at, uint64_t end, const BamRefs &R, BamMeasured &out) {
    static BamMeasured m[BamWaveHost::LANES];
    if (!on_wave(flt_at, [&](BamWaveHost &w) {
            BamMeasured &x = m[w.lane];
            x.rec = BamRec{0, 0, 0, 0, 0, 0}; x.line_len = 0; x.n_slices = 0;
            x.reason = bam_measure(w, b, at, end, R, x.rec, x.line_len, x.n_slices);
        })) return -6;
    for (uint32_t l = 1; l < BamWaveHost::LANES; ++l)
        if (m[l].reason != m[0].reason || m[l].n_slices != m[0].n_slices || m[l].line_len != m[0].line_len || m[l].rec.cigar_at != m[0].rec.cigar_at ||
            m[l].rec.cg_at != m[0].rec.cg_at || m[l].rec.seq_at != m[0].rec.seq_at || m[l].rec.cigar_len != m[0].rec.cigar_len || m[l].rec.n_cigar != m[0].rec.n_cigar)
            return -7;
    out = m[0];
    return 0;
}
static int write_on_wave(const uint8_t *b, uint64_t at, uint64_t end, const BamRefs &R, const BamRec &rec, uint32_t slice, const uint8_t *flt, uint8_t *dst,
                         uint64_t line_len) {
    static uint8_t ok[BamWaveHost::LANES];
    if (!on_wave(nullptr, [&](BamWaveHost &w) { ok[w.lane] = bam_write(w, b, at, end, R, rec, slice, flt, dst, line_len) ? 1u : 0u; })) return -6;
    for (uint32_t l = 1; l < BamWaveHost::LANES; ++l) if (ok[l] != ok[0]) return -7;
    return ok[0] ? 0 : -4;
}

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
    std::vector<BamRec> rec(n);
    std::vector<uint64_t> len(n);
    std::vector<uint32_t> slices(n), flt_first(n + 1u, 0u);
#ifdef BAM_HOST_MAIN
    // the program: every record on a copy of exactly its size, addressed from 0 (a look one byte behind a record is an error there even
    // when another record follows it in the file)
    std::vector<std::vector<uint8_t>> copy(n);
    for (uint32_t r = 0; r < n; ++r) copy[r].assign(b + off[r], b + off[r + 1u]);
#define BAM_HOST_REC(r) copy[r].data(), 0ull, (uint64_t)copy[r].size()
#else
#define BAM_HOST_REC(r) b, off[r], off[r + 1u]
#endif
    for (uint32_t r = 0; r < n; ++r) {
        flt_first[r] = (uint32_t)flt_at.size();
        BamMeasured m;
        if (const int rc = measure_on_wave(&flt_at, BAM_HOST_REC(r), R, m)) return rc;
        if (m.reason) {
            out->first_bad = r; out->first_bad_offset = off[r]; out->bad_reason = m.reason;
            return 0;
        }
        rec[r] = m.rec; len[r] = m.line_len; slices[r] = m.n_slices;
        if (!std::is_sorted(flt_at.begin() + flt_first[r], flt_at.end())) return -2;
#ifdef BAM_HOST_MAIN
        for (size_t k = flt_first[r]; k < flt_at.size(); ++k) flt_at[k] += off[r];
#endif
    }
    flt_first[n] = (uint32_t)flt_at.size();
    if (host_bad != ~0ull) { out->first_bad = host_bad; out->first_bad_offset = at; out->bad_reason = host_reason; return 0; }
    if (!std::is_sorted(flt_at.begin(), flt_at.end())) return -2;
    std::vector<uint8_t> slots(flt_at.size() * BAM_FLOAT_SLOT + 1u, 0);
    for (size_t k = 0; k < flt_at.size(); ++k) {
        if (flt_at[k] > at - 4u) return -2;
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
            if (const int rc = write_on_wave(BAM_HOST_REC(r), R, rec[r], k, slots.data() + (size_t)flt_first[r] * BAM_FLOAT_SLOT, dst, ll)) return rc;
        for (uint8_t *p = line.data(); p < dst; ++p) if (*p != 0xee) return -5;
        for (uint8_t *p = dst + ll; p < line.data() + line.size(); ++p) if (*p != 0xee) return -5;
        g_text.insert(g_text.end(), dst, dst + ll);
        g_line_off.push_back(g_text.size());
    }
    out->text = g_text.data(); out->line_off = g_line_off.data();
    out->n_records = n; out->n_text = g_text.size(); out->consumed = at;
    return 0;
}

// the store guards of bam_write (every store inside the line): the line of the first record of `bytes_in` (a good one; its float values
// through their slots, as in bam_host_to_sam) written into room that is longer than measured by one byte, or shorter — a line of up to
// 160 bytes cut at every byte, a longer one 1, 2, 3, 5, 8, 13 ... bytes in front of its end, behind the first byte of SEQ, and of no byte.  0: every call said that the line is not what was measured and
// stored nothing outside the room it was given; 1: the record is bad; -5: a byte outside was written; -8: a call took the wrong room
// for the right one
extern "C" int bam_host_guard(const uint8_t *bytes_in, uint64_t nbytes, const uint8_t *ref_names, const uint64_t *ref_off, uint32_t n_ref) {
    if (nbytes < 4u || !bytes_in) return -1;
    int32_t bs;
    memcpy(&bs, bytes_in, 4);
    if (bs < 0 || (uint64_t)bs > nbytes - 4u) return -1;
    const std::vector<uint8_t> exact(bytes_in, bytes_in + 4u + (uint64_t)bs), exact_names(ref_names, ref_names + (n_ref ? ref_off[n_ref] : 0));
    const BamRefs R{exact_names.data(), ref_off, n_ref};
    std::vector<uint64_t> flt_at;
    BamMeasured m;
    if (const int rc = measure_on_wave(&flt_at, exact.data(), 0, exact.size(), R, m)) return rc;
    if (m.reason) return 1;
    std::vector<uint8_t> slots(flt_at.size() * BAM_FLOAT_SLOT + BAM_FLOAT_SLOT, 0);          // the floats' text, as bam_host_to_sam makes it
    uint64_t ll = m.line_len;
    for (size_t k = 0; k < flt_at.size(); ++k) {
        if (flt_at[k] > exact.size() - 4u) return -2;
        float f;
        memcpy(&f, exact.data() + flt_at[k], 4);
        char buf[32];
        const int l = snprintf(buf, sizeof buf, "%g", (double)f);
        if (l < 0 || l > (int)BAM_FLOAT_CHARS) return -3;
        memcpy(&slots[k * BAM_FLOAT_SLOT], buf, (size_t)l);
        slots[k * BAM_FLOAT_SLOT + BAM_FLOAT_SLOT - 1u] = (uint8_t)l;
        ll += (uint64_t)l;
    }
    const uint64_t pad = 64;
    std::vector<uint64_t> rooms = {ll + 1u, m.rec.seq_at + 1u, 0u};
    if (ll <= 160u) for (uint64_t room = 1; room < ll; ++room) rooms.push_back(room);        // a short line: cut at every byte
    else for (uint64_t a = 1, b = 2; a <= ll; b += a, a = b - a) rooms.push_back(ll - a);    // cut 1, 2, 3, 5, 8, 13 ... bytes in front of the end: inside the tags
    for (const uint64_t room : rooms) {
        if (room == ll) continue;
        std::vector<uint8_t> line((size_t)(ll + 1u + 2u * pad + BAM_LANE_BYTES), 0xee);
        uint8_t *dst = line.data() + pad;
        dst += (BAM_LANE_BYTES - ((uintptr_t)dst & (BAM_LANE_BYTES - 1u))) & (BAM_LANE_BYTES - 1u);
        const int rc = write_on_wave(exact.data(), 0, exact.size(), R, m.rec, 0u, slots.data(), dst, room);
        if (rc != -4) return rc ? rc : -8;
        for (uint8_t *p = line.data(); p < line.data() + line.size(); ++p) if ((p < dst || p >= dst + room) && *p != 0xee) return -5;
    }
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
