// chain_guide_host.hip — TEST infrastructure (tests/test_chain_guide.py): the guide of the ECDF columns (guide_cell, ns_device.h; built by
// ns_pack.h) and the share of chain_error_list's iterations that leave its straight-line path, on the DEVICE source compiled for the host:
//   hipcc --cuda-host-only -x hip -O2 -std=c++17 -ffp-contract=off -DNS_HOST_TEST -shared -fPIC
// It includes ns_chain.h with the counting macro NS_CHAIN_COUNT, which no other build defines.  Nothing of the product links or loads this file.
#include <new>
#include <stdint.h>
static uint64_t g_chain_count[8];
#define NS_CHAIN_COUNT(what) (++g_chain_count[what])
#include "../nanosim_amd/csrc/ns_materialise.h"   // (wave_incl_scan: the cooperative chain of ns_chain.h, same include order as the engine)
#include "../nanosim_amd/csrc/ns_chain.h"
#include "../nanosim_amd/csrc/ns_pack.h"

struct GuideHost {
    ChainTab ct;
    std::vector<uint64_t> blob;
    bool whole;
};

extern "C" {

uint32_t cg_cells(void) { return NS_GUIDE_CELLS; }
uint32_t cg_octaves(void) { return NS_GUIDE_OCTAVES; }
void cg_cell(const uint32_t *u, uint32_t n, uint32_t *cell) { for (uint32_t i = 0; i < n; ++i) cell[i] = guide_cell(u[i]); }
uint32_t cg_cell_start(uint32_t cell) { return guide_cell_start(cell); }

void *cg_pack(const ns_model_tables *t) {
    GuideHost *h = new (std::nothrow) GuideHost;
    if (!h) return nullptr;
    ns_pack_chain_tables(t, t->mm_seg_off[t->mm_nbins], h->ct, h->blob, h->whole);
    return h;
}
void cg_free(void *p) { delete static_cast<GuideHost *>(p); }
uint32_t cg_lds_words(const void *p) { return static_cast<const GuideHost *>(p)->ct.n_words_lds; }
uint32_t cg_tail_bits(const void *p) { return static_cast<const GuideHost *>(p)->ct.tail_bits; }
int cg_whole(const void *p) { return static_cast<const GuideHost *>(p)->whole ? 1 : 0; }

// Every packed column (the first-match column, then every match-length column) against every draw: the true segment of a draw —
// #{s : p > hi[s]} on the fp64 edges of the model, found without a guide — must lie in [guide[cell], guide[cell + 1]] (the upper bound
// where the cell has a successor).  Returns the number of (column, draw) pairs that break a bound; *checked: pairs looked at.
uint64_t cg_bounds(const void *p, const ns_model_tables *t, const uint32_t *u, uint32_t n, uint64_t *checked) {
    const GuideHost *h = static_cast<const GuideHost *>(p);
    uint64_t bad = 0, seen = 0;
    for (uint32_t col = 0; col <= t->mm_nbins; ++col) {
        const uint32_t o = col ? t->mm_seg_off[col - 1] : 0u;
        const double *hi = col ? t->mm_hi + o : t->fm_hi;
        const uint32_t ns = col ? t->mm_seg_off[col] - o : t->fm_nseg;
        const uint16_t *g = reinterpret_cast<const uint16_t *>(h->blob.data() + (col ? h->ct.mm_guide : h->ct.fm_guide)) + (col ? NS_GUIDE_CELLS * (col - 1) : 0u);
        for (uint32_t i = 0; i < n; ++i) {
            const double pp = u32_to_p(u[i]);
            uint32_t lo = 0, up = ns;                                  // first s with !(p > hi[s])
            while (lo < up) { const uint32_t mid = (lo + up) >> 1; if (pp > hi[mid]) lo = mid + 1; else up = mid; }
            const uint32_t cell = guide_cell(u[i]);
            if (cell >= NS_GUIDE_CELLS || g[cell] > lo || (cell + 1u < NS_GUIDE_CELLS && lo > g[cell + 1u])) ++bad;
            ++seen;
        }
    }
    *checked = seen;
    return bad;
}

// chain_error_list on the LDS image (T = a copy of its words only) for one piece, events dropped (a sink without capacity only counts);
// counts[NS_CNT_N] gains the piece's iterations, calls of next_match_gv, narrow segments answered in place, draws with k1
void cg_count(const void *p, int32_t m_ref, uint64_t seed, uint64_t read, uint32_t seg, uint32_t attempt, uint64_t *counts) {
    const GuideHost *h = static_cast<const GuideHost *>(p);
    const Tabs TG{h->blob.data()};
    std::vector<uint64_t> lds(h->blob.begin(), h->blob.begin() + h->ct.n_words_lds);
    const Tabs T{lds.data()};
    const ns_key key{(uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)read, (uint32_t)(read >> 32)};
    EvSink32 s;
    s.ev = nullptr; s.cap = 0; s.n = 0; s.shift = 0; s.last_ins_len = 0; s.overflow = false; s.range = false; s.stg = nullptr; s.stride = 0;
    for (int k = 0; k < NS_CNT_N; ++k) g_chain_count[k] = 0;
    chain_error_list(T, TG, h->ct, m_ref, key, seg, attempt, s);
    for (int k = 0; k < NS_CNT_N; ++k) counts[k] += g_chain_count[k];
}

}  // extern "C"
