// chain_host.hip — TEST infrastructure: the thread-per-read event chains of the engine (nanosim_amd/csrc/ns_chain.h: chain_error_list,
// chain_error_list_g, chain_unaligned_error_list) and the table packing of ns_load_model (ns_pack.h) compiled for the HOST, so that `-m "not gpu"` tests can
// hold the device source against the oracle event by event (tests/test_chain_host.py).  Built by the test with
//   hipcc --cuda-host-only -x hip -O2 -std=c++17 -ffp-contract=off -DNS_HOST_TEST -shared -fPIC
// (host pass only: no device code, no HIP call).  Nothing of the product links or loads this file.
#include <new>
#include "../nanosim_amd/csrc/ns_materialise.h"   // (wave_incl_scan: the cooperative chain of ns_chain.h, same include order as the engine)
#include "../nanosim_amd/csrc/ns_chain.h"
#include "../nanosim_amd/csrc/ns_pack.h"

struct ChainHost {
    ChainTab ct;
    std::vector<uint64_t> blob;
    bool whole;
};

extern "C" {

void *chost_pack(const ns_model_tables *t) {
    ChainHost *h = new (std::nothrow) ChainHost;
    if (!h) return nullptr;
    ns_pack_chain_tables(t, t->mm_seg_off[t->mm_nbins], h->ct, h->blob, h->whole);
    return h;
}
void chost_free(void *p) { delete static_cast<ChainHost *>(p); }
int chost_whole(const void *p) { return static_cast<const ChainHost *>(p)->whole ? 1 : 0; }
uint32_t chost_lds_words(const void *p) { return static_cast<const ChainHost *>(p)->ct.n_words_lds; }
int chost_coop_ok(const ns_model_tables *t) { return ns_coop_ok(t, t->mm_seg_off[t->mm_nbins]) ? 1 : 0; }       // the gate of ns_load_model
uint32_t chost_tail_bits(const void *p) { return static_cast<const ChainHost *>(p)->ct.tail_bits; }

// variant 0: chain_error_list   — the integer image k_chain<LDS> walks (T = the blob's first n_words_lds words)
//         1: chain_error_list_g — the fp64 tables (models whose value edges are not whole numbers, tables too large for LDS)
//         2: chain_unaligned_error_list on the LDS image, 3: on the whole blob (k_chain<false, .>)
//         4: chain_error_list with the whole blob as its image (an integer image that does not fit LDS)
// T and TG: the LDS image is the first n_words_lds words of the blob — handing the chain a COPY of just those words as T checks that it
// never reads a table of the LDS part behind them.
// staged != 0: events go through the four-slot staging column (EvSink32::stg) as in k_chain<LDS> for single-piece reads; cap must then be
// a multiple of four and ev 32-byte aligned.  Returns 0, or -1 for an unknown variant.
int chost_error_list(const void *p, int variant, int staged, int32_t m_ref, uint64_t seed, uint64_t read, uint32_t seg, uint32_t attempt,
                     ns_event *ev, uint32_t cap, int32_t *l_new, int32_t *middle_ref, uint32_t *n_ev, int32_t *shift, int *overflow, int *range) {
    const ChainHost *h = static_cast<const ChainHost *>(p);
    const Tabs TG{h->blob.data()};
    std::vector<uint64_t> lds(h->blob.begin(), h->blob.begin() + h->ct.n_words_lds);      // (+ nothing: a read behind it is out of bounds)
    const Tabs T{lds.data()};
    const ns_key key{(uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)read, (uint32_t)(read >> 32)};
    uint2 stage[4 * NS_CHAIN_BLOCK];
    EvSink32 s;
    s.ev = ev; s.cap = cap; s.n = 0; s.shift = 0; s.last_ins_len = 0; s.overflow = false; s.range = false;
    s.stg = staged ? stage : nullptr; s.stride = NS_CHAIN_BLOCK;
    EList32 e;
    switch (variant) {
    case 0: e = chain_error_list(T, TG, h->ct, m_ref, key, seg, attempt, s); break;
    case 1: e = chain_error_list_g(TG, h->ct, m_ref, key, seg, attempt, s); break;
    case 2: e = chain_unaligned_error_list(T, h->ct, m_ref, key, seg, attempt, s); break;
    case 3: e = chain_unaligned_error_list(TG, h->ct, m_ref, key, seg, attempt, s); break;
    case 4: e = chain_error_list(TG, TG, h->ct, m_ref, key, seg, attempt, s); break;     // the integer image read from global memory (k_chain<false, false>)
    default: return -1;
    }
    ev_flush_tail(s);
    *l_new = e.l_new; *middle_ref = e.middle_ref; *n_ev = s.n; *shift = s.shift; *overflow = s.overflow; *range = s.range;
    return 0;
}

}  // extern "C"

#ifdef CHAIN_HOST_MAIN
// Stand-alone program for -fsanitize=address,undefined (tests/test_chain_edges.py): packs a model it makes up itself, every table in a heap
// buffer of exactly its size, so that a read or a store of the packer one element behind a table is an error; then builds the bucket
// table of one quality class into a buffer of exactly 1 024 entries.  Prints the image's size; exit status 0.
#include <cstdio>
int main() {
    const uint32_t nb = 3, nseg[3] = {4, 1, 6};
    std::vector<double> fm_hi{0.25, 0.5, 1.0}, fm_vhi{3, 9, 40};
    std::vector<int64_t> lo{0, 2, 7}, hi{2, 7, 200};       // (previous matches 200 .. 255 fall through the bin search to the last bin)
    std::vector<uint32_t> off{0, 4, 5, 11};
    std::vector<double> mm_hi, mm_vhi, vlo0{0, 1, 2};
    for (uint32_t b = 0; b < nb; ++b)
        for (uint32_t s = 0; s < nseg[b]; ++s) {
            mm_hi.push_back(s + 1 == nseg[b] ? (b == 2 ? 0.75 : 1.0) : (s + 1.0) / (nseg[b] + 1.0));       // (column 2: a last edge below the cut of every prefix)
            mm_vhi.push_back(vlo0[b] + (s + 1) * (b + 1) * 3);
        }
    std::vector<double> cdf[3][2];
    ns_model_tables *t = new ns_model_tables();
    t->fm_nseg = 3; t->fm_hi = fm_hi.data(); t->fm_vhi = fm_vhi.data(); t->fm_vlo0 = 0;
    t->mm_nbins = nb; t->mm_bin_lo = lo.data(); t->mm_bin_hi = hi.data(); t->mm_seg_off = off.data();
    t->mm_hi = mm_hi.data(); t->mm_vhi = mm_vhi.data(); t->mm_vlo0 = vlo0.data();
    for (int s = 0; s < 7; ++s) { t->trans[s][0] = 0.4; t->trans[s][1] = 0.7; t->trans[s][2] = 0.7; }
    for (int ty = 0; ty < 3; ++ty) {
        t->mix_w[ty] = 0.5;
        for (int c = 0; c < 2; ++c) {
            const uint32_t n = 1 + 3 * ty + c;
            for (uint32_t j = 0; j < n; ++j) cdf[ty][c].push_back(j + 1 == n ? (c ? 0.5 : 1.0) : (j + 1.0) / (2.0 * n));     // (component 1 ends below 1)
            t->mix_n[ty][c] = n; t->mix_cdf[ty][c] = cdf[ty][c].data();
        }
    }
    size_t words = 0;
    for (uint32_t force : {0u, 3u, 14u}) {
        ChainTab ct; std::vector<uint64_t> blob; bool whole = false;
        ns_pack_chain_tables(t, off[nb], ct, blob, whole, force);
        if (!whole || ct.n_words != blob.size()) return 1;
        words += blob.size();
    }
    std::vector<uint32_t> thr(NS_QUAL_LEVELS);
    for (uint32_t j = 0; j < NS_QUAL_LEVELS; ++j) thr[j] = j * 500u;
    std::vector<uint16_t> lut(1024);
    if (ns_qual_thr_decrease(thr.data())) return 2;
    ns_build_qual_lut(thr.data(), lut.data());
    printf("%zu words, lut[1023] %u\n", words, (unsigned)lut[1023]);
    delete t;
    return 0;
}
#endif
