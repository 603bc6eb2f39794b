// Test shim (CPU tests only): the engine's base-quality walk (nanosim_amd/csrc/ns_qual_hist.h — the code k_qual_mark runs per thread,
// and the classification and alignment look-up k_qual_count runs per byte) compiled for the HOST, behind the signature of
// ns_qual_histograms, so that the walk and the host module around the call are checked against the reference's fixture without a GPU.
// Marks are a byte per base here (the device packs 16 into a word).  Built by tests/test_basequal.py with g++ into tests/_tmp/.
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../include/nanosim_amd.h"
#include "../nanosim_amd/csrc/ns_qual_hist.h"

struct HostMarks {
    uint8_t *at;                                        // the first aligned base of the alignment
    void mark(uint64_t i, uint32_t m) { at[i] = (uint8_t)m; }
};

extern "C" int qh_host_histograms(void *, const uint8_t *cs, uint64_t, const uint64_t *cs_off, const uint8_t *qual, uint64_t qual_bytes,
                                  const uint64_t *qual_off, const ns_qual_aln *aln, uint32_t n_aln, ns_qual_hist *out) {
    memset(out, 0, sizeof *out);
    if (!n_aln) return 0;
    std::vector<uint8_t> marks(qual_bytes + 1, 0);
    for (uint32_t a = 0; a < n_aln; ++a) {                                      // mark phase
        const uint64_t len = qual_off[a + 1] - qual_off[a];
        if ((uint64_t)aln[a].head + aln[a].tail > len) return -1;
        const uint64_t aligned = len - aln[a].head - aln[a].tail;
        if (aln[a].unmapped || !aligned) continue;
        HostMarks sink{marks.data() + qual_off[a] + aln[a].head};
        const uint8_t *s = cs + cs_off[a];
        if (!qual_mark_alignment(s, cs_off[a + 1] - cs_off[a], aligned, sink)) out->n_short += 1;
    }
    uint32_t a = 0, next = 0;                                                   // count phase: byte by byte across the boundaries
    uint64_t lo = 0, hi = 0;
    for (uint64_t pos = qual_off[0]; pos < qual_off[n_aln]; ++pos) {
        if (pos >= hi) { a = qual_locate(qual_off, next, n_aln, pos); next = a + 1; lo = qual_off[a]; hi = qual_off[a + 1]; }
        const uint32_t q = (uint32_t)qual[pos] - NS_QUAL_FIRST;
        if (q >= NS_QUAL_VALUES) { out->n_bad_qual += 1; continue; }
        out->hist[qual_class(pos - lo, hi - lo, aln[a].head, aln[a].tail, aln[a].unmapped, marks[pos])][q] += 1;
    }
    return 0;
}
