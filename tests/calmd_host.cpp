// Test shim (CPU tests only): the engine's cs / MD walks (nanosim_amd/csrc/ns_calmd.h — the code the k_calmd_* kernels run per wavefront)
// compiled for the HOST behind the signature of ns_calmd, with a wavefront of ONE lane: the ballots are one bit, the prefix sums one term,
// a step one column and a round of the CIGAR one byte — the same code with 1 in the place of 64.  calmd_host_set_reference stands in
// for ns_set_reference: it keeps a copy normalised as the engine's (upper case, IUPAC codes and N with bit 7, anything else N).
// With -DCALMD_HOST_LANES=64 the wavefront has 64 lanes in lock step (tests/wave64_host.h; tests/test_calmd_wave64.py): the cross-lane
// arithmetic is then what the GPU runs.
// Built by tests/test_calmd.py with g++ into tests/_tmp/: as a shared library (ms_kernel: the wall time of the walks, one thread — what
// scripts/bench_characterize.py --calmd compares the GPU call with), and, with -DCALMD_HOST_MAIN, as a stand-alone program for
// -fsanitize=address,undefined.  The program gives every record its own copies, each of exactly its size — the CIGAR, the SEQ, the op
// table, the two texts, and the one chromosome it lies on — so that a read or a write beyond any of them is an error there:
// `calmd_host <file>` reads `C <bases>` lines (the chromosomes) and `R <cigar> <seq> <chrom> <pos>` lines (`~`: an empty string) and
// prints `n n_bad first_bad bad_reason` and a checksum of md, md_off, cs and cs_off.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <chrono>
#include <string>
#include <vector>
#include "../include/nanosim_amd.h"
#include "../nanosim_amd/csrc/ns_calmd.h"

#ifndef CALMD_HOST_LANES
#define CALMD_HOST_LANES 1
#endif
#if CALMD_HOST_LANES == 64
// -DCALMD_HOST_LANES=64: the same walks on the lock-step wavefront of tests/wave64_host.h, 64 host threads (-pthread), behind the same
// signatures.  Every lane keeps what the walk returns to it; the lanes have to agree, as on the GPU, where lane 0 stores it.
#include "wave64_host.h"
typedef Wave64Lane CalmdWaveHost;
static Wave64 g_wave;
template <class F> static bool on_wave(F f) { return g_wave.run([&](uint32_t lane) { CalmdWaveHost w{&g_wave, lane}; f(w); }); }
#elif CALMD_HOST_LANES == 1
struct CalmdWaveHost {
    static constexpr uint32_t LANES = 1u;
    uint32_t lane;
    uint64_t ballot(bool pred) const { return pred ? 1ull : 0ull; }
    uint64_t scan(uint64_t v, uint64_t &total) const { total = v; return 0u; }
    uint32_t bcast(uint32_t v, uint32_t) const { return v; }
    void fence() const {}
};
template <class F> static bool on_wave(F f) { CalmdWaveHost w{0u}; f(w); return true; }
#else
#error "CALMD_HOST_LANES is 1 or 64"
#endif

// calmd_measure and calmd_text<true> on the wave.  0; -6: the wave stopped (tests/wave64_host.h); -7: the lanes disagree on what the walk returns
struct CalmdMeasured { uint32_t reason; CalmdRec rec; uint64_t md_len, cs_len; };
static int measure_on_wave(const uint8_t *cg, uint64_t cn, const uint8_t *seq, uint64_t sn, uint32_t chrom, uint32_t pos, const CalmdRef &G, CalmdOp *T,
                           CalmdMeasured &out) {
    static CalmdMeasured m[CalmdWaveHost::LANES];
    if (!on_wave([&](CalmdWaveHost &w) {
            CalmdMeasured &x = m[w.lane];
            x.md_len = x.cs_len = 0;
            x.reason = calmd_measure(w, cg, cn, seq, sn, chrom, pos, G, T, x.rec, x.md_len, x.cs_len);
        })) return -6;
    for (uint32_t l = 1; l < CalmdWaveHost::LANES; ++l)
        if (m[l].reason != m[0].reason || m[l].md_len != m[0].md_len || m[l].cs_len != m[0].cs_len || m[l].rec.first_op != m[0].rec.first_op ||
            m[l].rec.end_op != m[0].rec.end_op || m[l].rec.n_cols != m[0].rec.n_cols || m[l].rec.reason != m[0].rec.reason) return -7;
    out = m[0];
    return 0;
}
static int write_on_wave(const CalmdOp *T, const CalmdRec &R, const uint8_t *seq, const uint8_t *ref, uint8_t *md, uint64_t md_len, uint8_t *cs, uint64_t cs_len) {
    static uint8_t ok[CalmdWaveHost::LANES];
    if (!on_wave([&](CalmdWaveHost &w) { uint64_t a = 0, b = 0; ok[w.lane] = calmd_text<true>(w, T, R, seq, ref, md, md_len, cs, cs_len, a, b) ? 1u : 0u; })) return -6;
    for (uint32_t l = 1; l < CalmdWaveHost::LANES; ++l) if (ok[l] != ok[0]) return -7;
    return ok[0] ? 0 : -4;
}

static std::vector<uint8_t> g_ref, g_md, g_cs;
static std::vector<uint64_t> g_chrom_off, g_md_off, g_cs_off;
static bool g_has_ref = false;

static uint8_t normalised(uint8_t c) {
    c &= 0x7fu;
    if (c >= 'a' && c <= 'z') c = (uint8_t)(c - 32);
    if (c == 'A' || c == 'C' || c == 'G' || c == 'T') return c;
    return (uint8_t)((strchr("YRWSKMDVHBNX", c) && c ? c : 'N') | 0x80u);
}

extern "C" uint32_t calmd_host_constant(int which) {
    const uint32_t v[] = {CALMD_MAX_DIGITS, CALMD_MAX_OPLEN, CALMD_SEQ_BYTES, (uint32_t)sizeof(CalmdOp)};
    return which >= 0 && which < 4 ? v[which] : 0u;
}

extern "C" int calmd_host_set_reference(const uint8_t *bases, uint64_t nbases, const uint64_t *chrom_off, uint32_t nchrom) {
    g_has_ref = false;
    if (!bases || !nbases || !chrom_off || !nchrom || chrom_off[nchrom] != nbases) return -1;
    g_ref.assign(bases, bases + nbases);
    for (uint8_t &b : g_ref) b = normalised(b);
    g_chrom_off.assign(chrom_off, chrom_off + nchrom + 1u);
    g_has_ref = true;
    return 0;
}

extern "C" int calmd_host(void *, const uint8_t *cigar, const uint64_t *cigar_off, const uint8_t *seq, const uint64_t *seq_off, const uint32_t *chrom,
                          const uint32_t *pos, uint32_t n, ns_calmd_result *out) {
    if (!out) return -1;
    out->md = out->cs = nullptr; out->md_off = out->cs_off = nullptr; out->n_bad = 0; out->first_bad = ~0ull; out->bad_reason = NS_CALMD_OK;
    out->reserved = 0; out->ms_kernel = 0;
    if (!g_has_ref || !cigar_off || !seq_off || (n && (!chrom || !pos)) || n >= (1u << 31) || cigar_off[0] || seq_off[0]) return -1;
    for (uint32_t i = 0; i < n; ++i) if (cigar_off[i] > cigar_off[i + 1u] || seq_off[i] > seq_off[i + 1u]) return -1;
    if ((cigar_off[n] && !cigar) || (seq_off[n] && !seq)) return -1;
    const uint32_t nchrom = (uint32_t)(g_chrom_off.size() - 1u);
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<CalmdRec> rec(n);
    g_md_off.assign((size_t)n + 1u, 0); g_cs_off.assign((size_t)n + 1u, 0);
#ifdef CALMD_HOST_MAIN
    // every record on copies of exactly its size; the reference: the one chromosome, addressed as the whole genome is
    g_md.clear(); g_cs.clear();
    for (uint32_t r = 0; r < n; ++r) {
        const std::vector<uint8_t> cg(cigar + cigar_off[r], cigar + cigar_off[r + 1u]), sq(seq + seq_off[r], seq + seq_off[r + 1u]);
        std::vector<CalmdOp> T(cg.size() / 2u);
        std::vector<uint8_t> chr;
        std::vector<uint64_t> off(g_chrom_off);
        CalmdRef G{nullptr, off.data(), nchrom};
        if (chrom[r] < nchrom) {
            chr.assign(g_ref.begin() + (ptrdiff_t)g_chrom_off[chrom[r]], g_ref.begin() + (ptrdiff_t)g_chrom_off[chrom[r] + 1u]);
            G.bases = reinterpret_cast<const uint8_t *>(reinterpret_cast<uintptr_t>(chr.data()) - (uintptr_t)g_chrom_off[chrom[r]]);
        }
        CalmdMeasured m;
        if (const int rc = measure_on_wave(cg.data(), cg.size(), sq.data(), sq.size(), chrom[r], pos[r], G, T.data(), m)) return rc;
        rec[r] = m.rec;
        const uint64_t ml = m.md_len, cl = m.cs_len;
        const uint32_t reason = m.reason;
        if (reason) { if (!out->n_bad++) { out->first_bad = r; out->bad_reason = reason; } if (ml || cl) return -2; }
        std::vector<uint8_t> md(ml), cs(cl);
        if (!reason)
            if (const int rc = write_on_wave(T.data(), rec[r], sq.data(), G.bases + g_chrom_off[chrom[r]] + (pos[r] - 1u), md.data(), ml, cs.data(), cl)) return rc;
        g_md.insert(g_md.end(), md.begin(), md.end()); g_cs.insert(g_cs.end(), cs.begin(), cs.end());
        g_md_off[r + 1u] = g_md.size(); g_cs_off[r + 1u] = g_cs.size();
    }
#else
    const CalmdRef G{g_ref.data(), g_chrom_off.data(), nchrom};
    std::vector<CalmdOp> T((size_t)(cigar_off[n] >> 1) + n + 1u);
    for (uint32_t r = 0; r < n; ++r) {
        CalmdMeasured m;
        if (const int rc = measure_on_wave(cigar + cigar_off[r], cigar_off[r + 1u] - cigar_off[r], seq + seq_off[r], seq_off[r + 1u] - seq_off[r], chrom[r], pos[r], G,
                                           T.data() + calmd_op_base(cigar_off, r), m)) return rc;
        rec[r] = m.rec;
        const uint64_t ml = m.md_len, cl = m.cs_len;
        const uint32_t reason = m.reason;
        if (reason) { if (!out->n_bad++) { out->first_bad = r; out->bad_reason = reason; } if (ml || cl) return -2; }
        g_md_off[r + 1u] = g_md_off[r] + ml; g_cs_off[r + 1u] = g_cs_off[r] + cl;
    }
    g_md.assign((size_t)g_md_off[n] + 1u, 0xee); g_cs.assign((size_t)g_cs_off[n] + 1u, 0xee);
    for (uint32_t r = 0; r < n; ++r) {
        if (rec[r].reason) continue;
        if (const int rc = write_on_wave(T.data() + calmd_op_base(cigar_off, r), rec[r], seq + seq_off[r], G.bases + g_chrom_off[chrom[r]] + (pos[r] - 1u),
                                         g_md.data() + g_md_off[r], g_md_off[r + 1u] - g_md_off[r], g_cs.data() + g_cs_off[r], g_cs_off[r + 1u] - g_cs_off[r])) return rc;
    }
    if (g_md.back() != 0xee || g_cs.back() != 0xee) return -5;
#endif
    out->ms_kernel = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (g_md.empty()) g_md.push_back(0);
    if (g_cs.empty()) g_cs.push_back(0);
    out->md = g_md.data(); out->cs = g_cs.data(); out->md_off = g_md_off.data(); out->cs_off = g_cs_off.data();
    return 0;
}

// the store guard of calmd_text<true> (every store inside the measured text, checked per lane): the texts of one good record written into
// room that is one byte shorter and one byte longer than measured, for MD and for cs in turn.  0: each of the four calls said that the
// texts are not what was measured and stored nothing outside the room it was given; 1: the record is bad; -5: a byte outside was written;
// -8: a call took the wrong room for the right one
extern "C" int calmd_host_guard(const uint8_t *cg, uint64_t cn, const uint8_t *seq, uint64_t sn, uint32_t chrom, uint32_t pos) {
    if (!g_has_ref) return -1;
    const CalmdRef G{g_ref.data(), g_chrom_off.data(), (uint32_t)(g_chrom_off.size() - 1u)};
    std::vector<CalmdOp> T((size_t)(cn >> 1) + 1u);
    CalmdMeasured m;
    if (const int rc = measure_on_wave(cg, cn, seq, sn, chrom, pos, G, T.data(), m)) return rc;
    if (m.reason) return 1;
    const uint8_t *ref = G.bases + g_chrom_off[chrom] + (pos - 1u);
    const uint64_t pad = 16;
    for (int v = 0; v < 4; ++v) {
        const uint64_t ml = m.md_len + (v == 0 ? ~0ull : v == 1 ? 1ull : 0ull), cl = m.cs_len + (v == 2 ? ~0ull : v == 3 ? 1ull : 0ull);
        if ((v == 0 && !m.md_len) || (v == 2 && !m.cs_len)) continue;
        std::vector<uint8_t> md((size_t)(m.md_len + 1u + 2u * pad), 0xee), cs((size_t)(m.cs_len + 1u + 2u * pad), 0xee);
        const int rc = write_on_wave(T.data(), m.rec, seq, ref, md.data() + pad, ml, cs.data() + pad, cl);
        if (rc != -4) return rc ? rc : -8;
        for (size_t i = 0; i < md.size(); ++i) if ((i < pad || i >= pad + ml) && md[i] != 0xee) return -5;
        for (size_t i = 0; i < cs.size(); ++i) if ((i < pad || i >= pad + cl) && cs[i] != 0xee) return -5;
    }
    return 0;
}

#ifdef CALMD_HOST_MAIN
#include <stdlib.h>
#include <fstream>
#include <sstream>
int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::ifstream f(argv[1]);
    if (!f) return 2;
    std::vector<uint8_t> bases, cigar, seq;
    std::vector<uint64_t> chrom_off{0}, cigar_off{0}, seq_off{0};
    std::vector<uint32_t> chrom, pos;
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream in(line);
        std::string kind, a, b;
        in >> kind;
        if (kind == "C") { in >> a; bases.insert(bases.end(), a.begin(), a.end()); chrom_off.push_back(bases.size()); }
        else if (kind == "R") {
            unsigned long c = 0, p = 0;
            in >> a >> b >> c >> p;
            if (a == "~") a.clear();
            if (b == "~") b.clear();
            cigar.insert(cigar.end(), a.begin(), a.end()); cigar_off.push_back(cigar.size());
            seq.insert(seq.end(), b.begin(), b.end()); seq_off.push_back(seq.size());
            chrom.push_back((uint32_t)c); pos.push_back((uint32_t)p);
        }
    }
    if (calmd_host_set_reference(bases.data(), bases.size(), chrom_off.data(), (uint32_t)(chrom_off.size() - 1u))) return 3;
    ns_calmd_result out;
    const uint32_t n = (uint32_t)chrom.size();
    const int rc = calmd_host(nullptr, cigar.data(), cigar_off.data(), seq.data(), seq_off.data(), chrom.data(), pos.data(), n, &out);
    if (rc) return 4;
    unsigned long long sum = 0;
    for (uint64_t i = 0; i < out.md_off[n]; ++i) sum = sum * 31u + out.md[i];
    for (uint64_t i = 0; i <= n; ++i) sum = sum * 31u + out.md_off[i];
    for (uint64_t i = 0; i < out.cs_off[n]; ++i) sum = sum * 31u + out.cs[i];
    for (uint64_t i = 0; i <= n; ++i) sum = sum * 31u + out.cs_off[i];
    printf("%u %llu %lld %u\n%llu\n", n, (unsigned long long)out.n_bad, (long long)out.first_bad, out.bad_reason, sum);
    return 0;
}
#endif
