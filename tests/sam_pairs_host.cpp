// Test shim (CPU tests only): the engine's SAM walk (nanosim_amd/csrc/ns_sam_pairs.h — the code k_sam_scan and k_sam_lines run per
// thread) compiled for the HOST behind the signatures of ns_sam_pairs_build and ns_hp_histograms_sam, so that the walk and the host
// module around the calls are checked against the reference's fixture without a GPU.  The homopolymer walk behind the second call is
// the shim of tests/hp_train_host.cpp.  Built by tests/test_sam_pairs.py with g++ into tests/_tmp/.
#include <stdint.h>
#include <string.h>
#include <vector>
#include "hp_train_host.cpp"
#include "../nanosim_amd/csrc/ns_sam_pairs.h"

static bool offsets_ok(const uint64_t *off, uint32_t n) {
    for (uint32_t a = 0; a < n; ++a) if (off[a] > off[a + 1]) return false;
    return true;
}

extern "C" int sam_host_pairs_build(void *, const uint8_t *cigar, const uint64_t *cigar_off, const uint8_t *md, const uint64_t *md_off,
                                    const uint8_t *seq, const uint64_t *seq_off, uint32_t n_aln, ns_sam_pairs *out) {
    if (!out || !out->aln_off || (!out->ref_lines != !out->query_lines)) return -1;
    if (n_aln && (!cigar_off || !md_off || !seq_off || !offsets_ok(cigar_off, n_aln) || !offsets_ok(md_off, n_aln) || !offsets_ok(seq_off, n_aln))) return -1;
    out->n_bytes = out->n_bad = 0; out->first_bad = n_aln; out->ms_kernel = 0;
    out->aln_off[0] = 0;
    if (!n_aln) return 0;
    // phase 1: every record's figures and exceptions, each list at the place the device gives it
    std::vector<SamExc> exc((size_t)sam_exc_base(cigar_off, md_off, n_aln));
    std::vector<uint32_t> n_exc(n_aln), head(n_aln);
    for (uint32_t a = 0; a < n_aln; ++a) {
        const uint8_t *c = cigar + cigar_off[a], *m = md + md_off[a];
        const uint64_t sn = seq_off[a + 1] - seq_off[a];
        SamFigures F;
        const bool ok = sam_scan_record(c, cigar_off[a + 1] - cigar_off[a], m, md_off[a + 1] - md_off[a], sn, sn == 1 && seq[seq_off[a]] == '*',
                                        exc.data() + sam_exc_base(cigar_off, md_off, a), F);
        if (!ok) { if (!out->n_bad) out->first_bad = a; out->n_bad += 1; }
        if (out->aln) out->aln[a] = ns_sam_aln{F.head, F.tail, F.ref_len, F.query_len};
        n_exc[a] = F.n_exc; head[a] = F.head;
        out->aln_off[a + 1] = out->aln_off[a] + F.cols;
    }
    out->n_bytes = out->aln_off[n_aln];
    if (!out->ref_lines || out->n_bytes > out->cap_bytes) return 0;
    // phase 2: every column through the cursor the device uses — from a search at every 16th column, as a thread of k_sam_lines begins
    for (uint32_t a = 0; a < n_aln; ++a) {
        const SamExc *x = exc.data() + sam_exc_base(cigar_off, md_off, a);
        const uint64_t lo = out->aln_off[a], n = out->aln_off[a + 1] - lo;
        SamCursor k;
        for (uint64_t c = 0; c < n; ++c) {
            if ((lo + c) % 16u == 0 || c == 0) sam_cursor_at(k, x, n_exc[a], (uint32_t)c);
            sam_column(k, x, n_exc[a], (uint32_t)c, seq, seq_off[a] + head[a], md, md_off[a], out->ref_lines[lo + c], out->query_lines[lo + c]);
        }
    }
    return 0;
}

extern "C" int sam_host_hp_histograms_sam(void *, const uint8_t *cigar, const uint64_t *cigar_off, const uint8_t *md, const uint64_t *md_off,
                                          const uint8_t *seq, const uint64_t *seq_off, uint32_t n_aln, uint32_t min_hp_len, ns_sam_pairs *pairs,
                                          ns_hp_hist *out) {
    if (!out || !out->table || !min_hp_len || !out->cap_ref || !out->cap_read) return -1;
    std::vector<uint64_t> off((size_t)n_aln + 1);
    ns_sam_pairs size;
    memset(&size, 0, sizeof size);
    size.aln_off = off.data();
    if (int rc = sam_host_pairs_build(nullptr, cigar, cigar_off, md, md_off, seq, seq_off, n_aln, &size)) return rc;
    std::vector<uint8_t> ref((size_t)size.n_bytes + 1), qry((size_t)size.n_bytes + 1);
    size.ref_lines = ref.data(); size.query_lines = qry.data(); size.cap_bytes = size.n_bytes;
    if (int rc = sam_host_pairs_build(nullptr, cigar, cigar_off, md, md_off, seq, seq_off, n_aln, &size)) return rc;
    if (pairs) if (int rc = sam_host_pairs_build(nullptr, cigar, cigar_off, md, md_off, seq, seq_off, n_aln, pairs)) return rc;
    out->n_hp = out->max_ref = out->max_read = out->n_overflow = 0; out->ms_kernel = 0;
    memset(out->columns, 0, sizeof out->columns);
    memset(out->table, 0, (size_t)2 * out->cap_ref * out->cap_read * 8);
    if (size.n_bad) return 0;
    return hp_host_histograms(nullptr, ref.data(), qry.data(), size.n_bytes, off.data(), n_aln, min_hp_len, out);
}
