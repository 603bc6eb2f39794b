// Test shim (CPU tests only): the engine's CIGAR walk and segment rule (nanosim_amd/csrc/ns_read_len.h — the code k_len_scan and
// k_len_flag run per thread) compiled for the HOST behind the signature of ns_read_lengths, so that the walk, the rule and the host
// module around the call are checked against the reference's fixture without a GPU.  The reduction — atomics on the device — is the
// serial loop here.  Built by tests/test_read_lengths.py with g++ into tests/_tmp/: as a shared library, and, with -DREAD_LEN_MAIN, as
// a stand-alone program for -fsanitize=address,undefined that reads records from a text file:
//   n_refs, then LN per reference; then per record `first_of_read reverse ref_id ref_start cigar` (cigar `-` = empty)
// and prints `n_segments n_bad first_bad` and a checksum of everything it wrote.
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../include/nanosim_amd.h"
#include "../nanosim_amd/csrc/ns_read_len.h"

extern "C" int len_host_read_lengths(void *, const uint8_t *cigar, const uint64_t *cigar_off, const uint8_t *reverse, const uint32_t *ref_id,
                                     const uint64_t *ref_start, const uint64_t *ref_total, uint32_t n_refs, const uint64_t *read_off, uint32_t n_reads,
                                     uint32_t n_aln, int mode, const uint32_t *extra_head, const uint32_t *extra_tail, ns_len_result *out) {
    if (!out || !read_off || (n_reads && !out->reads) || (!extra_head != !extra_tail)) return -1;
    if (n_aln && (!out->segments || !cigar_off || !reverse || !ref_id || !ref_start || !ref_total)) return -1;
    if (mode != NS_LEN_GENOME && mode != NS_LEN_TRANSCRIPTOME) return -1;
    out->n_segments = out->n_bad = 0; out->first_bad = n_aln; out->ms_kernel = 0;
    for (uint32_t r = 0; r < n_reads; ++r) if (read_off[r] >= read_off[r + 1]) return -1;
    if (read_off[0] != 0 || read_off[n_reads] != n_aln) return -1;
    for (uint32_t a = 0; a < n_aln; ++a) if (cigar_off[a] > cigar_off[a + 1] || ref_id[a] >= n_refs) return -1;
    std::vector<LenFigures> fig(n_aln);
    for (uint32_t a = 0; a < n_aln; ++a) {
        const uint8_t *c = cigar + cigar_off[a];
        const bool ok = len_scan_record(c, cigar_off[a + 1] - cigar_off[a], reverse[a] != 0, ref_start[a], ref_total[ref_id[a]], fig[a]);
        if (!ok) { if (!out->n_bad) out->first_bad = a; out->n_bad += 1; }
        if (out->aln) out->aln[a] = ns_len_aln{fig[a].head, fig[a].tail, fig[a].read_len, fig[a].ref_len, fig[a].query_aln_len, fig[a].edge};
    }
    for (uint32_t r = 0; r < n_reads; ++r) {
        ns_len_read R{0u, extra_head ? extra_head[r] : NS_LEN_NONE, extra_tail ? extra_tail[r] : NS_LEN_NONE, 0u};
        const uint64_t first = read_off[r];
        for (uint64_t a = first; a < read_off[r + 1]; ++a) {
            const bool is_first = a == first;
            if (len_starts_segment(mode, is_first, !is_first && ref_id[a - 1] == ref_id[a], fig[first].edge, fig[a].edge)) {
                out->segments[out->n_segments++] = 0;
                R.n_segments += 1;
            }
            out->segments[out->n_segments - 1] += fig[a].ref_len;
            if (fig[a].read_len > R.read_len) R.read_len = fig[a].read_len;
            if (fig[a].head < R.head) R.head = fig[a].head;
            if (fig[a].tail < R.tail) R.tail = fig[a].tail;
        }
        out->reads[r] = R;
    }
    return 0;
}

#ifdef READ_LEN_MAIN
#include <stdio.h>
#include <string>
int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    unsigned n_refs = 0;
    if (fscanf(f, "%u", &n_refs) != 1) return 2;
    std::vector<uint64_t> total(n_refs);
    for (unsigned i = 0; i < n_refs; ++i) { unsigned long long v; if (fscanf(f, "%llu", &v) != 1) return 2; total[i] = v; }
    std::vector<uint8_t> cigar, reverse; std::vector<uint64_t> off{0}, start, read_off; std::vector<uint32_t> ref_id;
    std::vector<char> buf(1 << 20);
    unsigned first, rev, rid; unsigned long long st;
    while (fscanf(f, "%u %u %u %llu %1048575s", &first, &rev, &rid, &st, buf.data()) == 5) {
        if (first) read_off.push_back(start.size());
        const std::string c = strcmp(buf.data(), "-") ? buf.data() : "";
        cigar.insert(cigar.end(), c.begin(), c.end());               // (no padding behind the bytes: a read beyond them is an error here)
        off.push_back(cigar.size()); reverse.push_back((uint8_t)rev); ref_id.push_back(rid); start.push_back(st);
    }
    fclose(f);
    read_off.push_back(start.size());
    const uint32_t n_aln = (uint32_t)start.size(), n_reads = (uint32_t)read_off.size() - 1;
    unsigned long long sum = 0;
    for (int mode = 0; mode < 2; ++mode) {
        std::vector<ns_len_aln> aln(n_aln); std::vector<ns_len_read> reads(n_reads); std::vector<uint64_t> seg(n_aln);
        ns_len_result out;
        memset(&out, 0, sizeof out);
        out.aln = aln.data(); out.reads = reads.data(); out.segments = seg.data();
        std::vector<uint8_t> exact(cigar);                            // (an exact-size copy: the sanitizer sees a byte read past the end)
        if (len_host_read_lengths(nullptr, exact.data(), off.data(), reverse.data(), ref_id.data(), start.data(), total.data(), n_refs, read_off.data(),
                                  n_reads, n_aln, mode, nullptr, nullptr, &out)) return 3;
        for (uint64_t i = 0; i < out.n_segments; ++i) sum = sum * 31u + seg[i];
        for (const ns_len_read &r : reads) sum = sum * 31u + r.read_len + 7ull * r.head + 13ull * r.tail + 17ull * r.n_segments;
        for (const ns_len_aln &a : aln) sum = sum * 31u + a.query_aln_len + 3ull * a.edge;
        printf("%llu %llu %llu\n", (unsigned long long)out.n_segments, (unsigned long long)out.n_bad, (unsigned long long)out.first_bad);
    }
    printf("%llu\n", sum);
    return 0;
}
#endif
