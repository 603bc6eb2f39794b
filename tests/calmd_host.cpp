// Test shim (CPU tests only): the engine's cs / MD walks (nanosim_amd/csrc/ns_calmd.h — the code the k_calmd_* kernels run per wavefront)
// compiled for the HOST behind the signature of ns_calmd, with a wavefront of ONE lane: the ballots are one bit, the prefix sums one term,
// a step one column and a round of the CIGAR one byte — the same code with 1 in the place of 64.  calmd_host_set_reference stands in
// for ns_set_reference: it keeps a copy normalised as the engine's (upper case, IUPAC codes and N with bit 7, anything else N).
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

struct CalmdWaveHost {
    static constexpr uint32_t LANES = 1u;
    uint32_t lane;
    uint64_t ballot(bool pred) const { return pred ? 1ull : 0ull; }
    uint64_t scan(uint64_t v, uint64_t &total) const { total = v; return 0u; }
    uint32_t bcast(uint32_t v, uint32_t) const { return v; }
    void fence() const {}
};

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
    CalmdWaveHost w{0u};
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
        uint64_t ml = 0, cl = 0;
        const uint32_t reason = calmd_measure(w, cg.data(), cg.size(), sq.data(), sq.size(), chrom[r], pos[r], G, T.data(), rec[r], ml, cl);
        if (reason) { if (!out->n_bad++) { out->first_bad = r; out->bad_reason = reason; } if (ml || cl) return -2; }
        std::vector<uint8_t> md(ml), cs(cl);
        if (!reason) {
            uint64_t a = 0, b = 0;
            if (!calmd_text<true>(w, T.data(), rec[r], sq.data(), G.bases + g_chrom_off[chrom[r]] + (pos[r] - 1u), md.data(), ml, cs.data(), cl, a, b)) return -4;
        }
        g_md.insert(g_md.end(), md.begin(), md.end()); g_cs.insert(g_cs.end(), cs.begin(), cs.end());
        g_md_off[r + 1u] = g_md.size(); g_cs_off[r + 1u] = g_cs.size();
    }
#else
    const CalmdRef G{g_ref.data(), g_chrom_off.data(), nchrom};
    std::vector<CalmdOp> T((size_t)(cigar_off[n] >> 1) + n + 1u);
    for (uint32_t r = 0; r < n; ++r) {
        uint64_t ml = 0, cl = 0;
        const uint32_t reason = calmd_measure(w, cigar + cigar_off[r], cigar_off[r + 1u] - cigar_off[r], seq + seq_off[r], seq_off[r + 1u] - seq_off[r], chrom[r],
                                              pos[r], G, T.data() + calmd_op_base(cigar_off, r), rec[r], ml, cl);
        if (reason) { if (!out->n_bad++) { out->first_bad = r; out->bad_reason = reason; } if (ml || cl) return -2; }
        g_md_off[r + 1u] = g_md_off[r] + ml; g_cs_off[r + 1u] = g_cs_off[r] + cl;
    }
    g_md.assign((size_t)g_md_off[n] + 1u, 0xee); g_cs.assign((size_t)g_cs_off[n] + 1u, 0xee);
    for (uint32_t r = 0; r < n; ++r) {
        if (rec[r].reason) continue;
        uint64_t a = 0, b = 0;
        if (!calmd_text<true>(w, T.data() + calmd_op_base(cigar_off, r), rec[r], seq + seq_off[r], G.bases + g_chrom_off[chrom[r]] + (pos[r] - 1u),
                              g_md.data() + g_md_off[r], g_md_off[r + 1u] - g_md_off[r], g_cs.data() + g_cs_off[r], g_cs_off[r + 1u] - g_cs_off[r], a, b)) return -4;
    }
    if (g_md.back() != 0xee || g_cs.back() != 0xee) return -5;
#endif
    out->ms_kernel = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (g_md.empty()) g_md.push_back(0);
    if (g_cs.empty()) g_cs.push_back(0);
    out->md = g_md.data(); out->cs = g_cs.data(); out->md_off = g_md_off.data(); out->cs_off = g_cs_off.data();
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
