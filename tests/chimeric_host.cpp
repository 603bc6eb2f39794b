// Test shim (CPU tests only): the engine's CIGAR reading and split-alignment choice (nanosim_amd/csrc/ns_chimeric.h — the code
// k_chim_scan and k_chim_select run per thread) compiled for the HOST behind the signatures of ns_cigar_spans and ns_chimeric_select, so
// that the walk and the host module around the calls are checked against the reference's fixture without a GPU.  The sums — wavefront
// sums and atomics on the device — are serial loops here.  Built by tests/test_chimeric_train.py with g++ into tests/_tmp/: as a shared
// library, and, with -DCHIMERIC_MAIN, as a stand-alone program for -fsanitize=address,undefined that reads entries from a text file:
//   n_refs, then `LN species` per reference; then per entry `first_of_read reverse ref_id ref_start nm cigar` (cigar `-` = empty)
// and prints `n_gaps pos_strand n_bad first_bad` and a checksum of everything it wrote.
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../include/nanosim_amd.h"
#include "../nanosim_amd/csrc/ns_chimeric.h"

static_assert(sizeof(ChimFigures) == sizeof(ns_chim_ent) && sizeof(ChimPiece) == sizeof(ns_chim_piece), "ns_chimeric.h mirrors the ABI structs");

extern "C" int chim_host_cigar_spans(void *, const uint8_t *cigar, const uint64_t *cigar_off, uint32_t n, ns_chim_ent *out, uint64_t *n_bad,
                                     uint64_t *first_bad, double *ms_kernel) {
    if (!n_bad || !first_bad || !ms_kernel || (n && (!cigar_off || !out))) return -1;
    *n_bad = 0; *first_bad = n; *ms_kernel = 0;
    for (uint32_t a = 0; a < n; ++a) if (cigar_off[a] > cigar_off[a + 1]) return -1;
    for (uint32_t a = 0; a < n; ++a) {
        const uint8_t *c = cigar + cigar_off[a];
        ChimFigures F;
        if (!chim_scan_cigar(c, cigar_off[a + 1] - cigar_off[a], CHIM_PARSER, F)) { if (!*n_bad) *first_bad = a; *n_bad += 1; }
        out[a] = ns_chim_ent{F.qstart, F.qend, F.qlen, F.rlen};
    }
    return 0;
}

struct ChimHostAdd { void operator()(unsigned long long *p, unsigned long long v) const { *p += v; } };

extern "C" int chim_host_chimeric_select(void *, const uint8_t *cigar, const uint64_t *cigar_off, const uint64_t *ent_off, uint32_t n_reads,
                                         const uint32_t *ref_id, const uint64_t *ref_start, const uint32_t *nm, const uint8_t *reverse,
                                         const uint64_t *ref_total, const uint32_t *species, uint32_t n_refs, uint32_t n_species, ns_chim_result *out) {
    if (!out || !ent_off || (n_species && !out->species_count)) return -1;
    out->n_gaps = out->pos_strand = out->n_bad = 0; out->first_bad = 0; out->ms_kernel = out->ms_scan = 0;
    if (ent_off[0] != 0) return -1;
    for (uint32_t r = 0; r < n_reads; ++r) if (ent_off[r] >= ent_off[r + 1]) return -1;
    const uint32_t n_ent = (uint32_t)ent_off[n_reads];
    out->first_bad = n_ent;
    for (uint32_t i = 0; i < 2u * n_species; ++i) out->species_count[i] = 0;
    if (n_refs && (!ref_total || !species)) return -1;
    for (uint32_t i = 0; i < n_refs; ++i) if (species[i] >= n_species) return -1;
    if (!n_reads) return 0;
    if (!out->reads || !out->pieces || !cigar_off || !ref_id || !ref_start || !nm || !reverse) return -1;
    for (uint32_t a = 0; a < n_ent; ++a) if (cigar_off[a] > cigar_off[a + 1] || ref_id[a] >= n_refs) return -1;
    std::vector<ChimFigures> fig(n_ent);
    std::vector<uint8_t> primary(n_ent, 0);
    for (uint32_t r = 0; r < n_reads; ++r) primary[ent_off[r]] = 1;
    for (uint32_t a = 0; a < n_ent; ++a) {
        const uint8_t *c = cigar + cigar_off[a];
        if (!chim_scan_cigar(c, cigar_off[a + 1] - cigar_off[a], primary[a] ? CHIM_PYSAM : CHIM_PARSER, fig[a])) { if (!out->n_bad) out->first_bad = a; out->n_bad += 1; }
        if (out->ent) out->ent[a] = ns_chim_ent{fig[a].qstart, fig[a].qend, fig[a].qlen, fig[a].rlen};
    }
    std::vector<unsigned long long> count((size_t)2 * n_species, 0ull);
    ChimHostAdd add;
    for (uint32_t r = 0; r < n_reads; ++r) {
        const uint64_t e0 = ent_off[r], n = ent_off[r + 1] - e0;
        std::vector<uint64_t> ws(chim_ws_words(n), 0xa5a5a5a5a5a5a5a5ull);           // (exactly the words the header asks for, not zeroed)
        std::vector<ChimPiece> pieces(n);
        ChimTotals T; uint32_t flags = 0;
        const uint32_t k = chim_select_read(n, fig.data() + e0, ref_id + e0, ref_start + e0, nm + e0, reverse + e0, ref_total, species, ws.data(),
                                            pieces.data(), count.data(), add, T, flags);
        out->reads[r] = ns_chim_read{k, flags};
        for (uint64_t i = 0; i < n; ++i)
            out->pieces[e0 + i] = i < k ? ns_chim_piece{pieces[i].entry, pieces[i].is_primary, pieces[i].gap} : ns_chim_piece{0u, 0u, 0};
        out->n_gaps += T.n_gaps; out->pos_strand += T.pos_strand;
        // "ws: contents undefined": the same read over a zeroed workspace has to choose the same (a walk that looks at a list it has
        // not opened yet finds the primary in the pattern above and nothing here)
        std::vector<uint64_t> ws0(chim_ws_words(n), 0ull);
        std::vector<ChimPiece> pieces0(n);
        std::vector<unsigned long long> count0((size_t)2 * n_species, 0ull);
        ChimTotals T0; uint32_t flags0 = 0;
        const uint32_t k0 = chim_select_read(n, fig.data() + e0, ref_id + e0, ref_start + e0, nm + e0, reverse + e0, ref_total, species, ws0.data(),
                                             pieces0.data(), count0.data(), add, T0, flags0);
        if (k0 != k || flags0 != flags || T0.n_gaps != T.n_gaps || T0.pos_strand != T.pos_strand) return -2;
        for (uint32_t i = 0; i < k; ++i)
            if (pieces0[i].entry != pieces[i].entry || pieces0[i].is_primary != pieces[i].is_primary || pieces0[i].gap != pieces[i].gap) return -2;
    }
    for (uint32_t i = 0; i < 2u * n_species; ++i) out->species_count[i] = count[i];
    return 0;
}

#ifdef CHIMERIC_MAIN
#include <stdio.h>
#include <string>
int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    unsigned n_refs = 0, n_species = 0;
    if (fscanf(f, "%u", &n_refs) != 1) return 2;
    std::vector<uint64_t> total(n_refs); std::vector<uint32_t> species(n_refs);
    for (unsigned i = 0; i < n_refs; ++i) {
        unsigned long long v; unsigned sp;
        if (fscanf(f, "%llu %u", &v, &sp) != 2) return 2;
        total[i] = v; species[i] = sp; if (sp + 1 > n_species) n_species = sp + 1;
    }
    std::vector<uint8_t> cigar, reverse; std::vector<uint64_t> off{0}, start, ent_off; std::vector<uint32_t> ref_id, nm;
    std::vector<char> buf(1 << 20);
    unsigned first, rev, rid, n_m; unsigned long long st;
    while (fscanf(f, "%u %u %u %llu %u %1048575s", &first, &rev, &rid, &st, &n_m, buf.data()) == 6) {
        if (first) ent_off.push_back(start.size());
        const std::string c = strcmp(buf.data(), "-") ? buf.data() : "";
        cigar.insert(cigar.end(), c.begin(), c.end());               // (no padding behind the bytes: a read beyond them is an error here)
        off.push_back(cigar.size()); reverse.push_back((uint8_t)rev); ref_id.push_back(rid); start.push_back(st); nm.push_back(n_m);
    }
    fclose(f);
    ent_off.push_back(start.size());
    const uint32_t n_ent = (uint32_t)start.size(), n_reads = (uint32_t)ent_off.size() - 1;
    std::vector<ns_chim_ent> ent(n_ent), spans(n_ent); std::vector<ns_chim_piece> pieces(n_ent); std::vector<ns_chim_read> reads(n_reads);
    std::vector<uint64_t> count((size_t)2 * n_species);
    ns_chim_result out;
    memset(&out, 0, sizeof out);
    out.ent = ent.data(); out.pieces = pieces.data(); out.reads = reads.data(); out.species_count = count.data();
    std::vector<uint8_t> exact(cigar);                                // (an exact-size copy: the sanitizer sees a byte read past the end)
    if (chim_host_chimeric_select(nullptr, exact.data(), off.data(), ent_off.data(), n_reads, ref_id.data(), start.data(), nm.data(), reverse.data(),
                                  total.data(), species.data(), n_refs, n_species, &out)) return 3;
    uint64_t nb = 0, fb = 0; double ms = 0;
    if (chim_host_cigar_spans(nullptr, exact.data(), off.data(), n_ent, spans.data(), &nb, &fb, &ms)) return 3;
    unsigned long long sum = 0;
    for (const ns_chim_ent &e : ent) sum = sum * 31u + e.qstart + 3ull * e.qend + 5ull * e.rlen;
    for (const ns_chim_ent &e : spans) sum = sum * 31u + e.qstart + 3ull * e.qend + 5ull * e.rlen;
    for (uint32_t r = 0; r < n_reads; ++r) {
        sum = sum * 31u + reads[r].n_pieces + 7ull * reads[r].flags;
        for (uint32_t i = 0; i < reads[r].n_pieces; ++i) { const ns_chim_piece &p = pieces[ent_off[r] + i]; sum = sum * 31u + p.entry + 3ull * p.is_primary + 11ull * (uint64_t)p.gap; }
    }
    for (uint64_t c : count) sum = sum * 31u + c;
    printf("%llu %llu %llu %llu\n", (unsigned long long)out.n_gaps, (unsigned long long)out.pos_strand, (unsigned long long)out.n_bad, (unsigned long long)out.first_bad);
    printf("%llu %llu\n%llu\n", (unsigned long long)nb, (unsigned long long)fb, sum);
    return 0;
}
#endif
