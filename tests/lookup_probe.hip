// lookup_probe.hip — TEST infrastructure: the table look-ups of the event chains (nanosim_amd/csrc/ns_chain.h: ecdf_lookup_gv, next_match_gv
// with ecdf_lookup_pre, ecdf_lookup_g, run_length_r, run_length_t; trans_pick_u of ns_device.h) on a model packed by ns_pack_chain_tables
// (ns_pack.h), evaluated DRAW BY DRAW over arrays of inputs, so that tests/test_lookup_probe.py can put draws on and next to every threshold
// of the packed image and hold each answer against the oracle's fp64 arithmetic.  Built by the test twice, into a temporary directory:
//   for gfx950:    hipcc <the engine's HIP_FLAGS>                                   one bounds-checked kernel per look-up
//   for the host:  hipcc --cuda-host-only -x hip -O2 -std=c++17 -ffp-contract=off -DNS_HOST_TEST -shared -fPIC   the same functions in a loop
// T is the LDS part of the blob and TG the whole blob, as k_chain has them: on the host T is a COPY of exactly n_words_lds words (a read
// behind a prefix table is out of bounds), on the GPU the kernel copies those words into LDS while they fit, else reads a buffer of just them.
// Nothing of the product links or loads this file.
#include <new>
#include "../nanosim_amd/csrc/ns_materialise.h"   // (wave_incl_scan: the cooperative chain of ns_chain.h, same include order as the engine)
#include "../nanosim_amd/csrc/ns_chain.h"
#include "../nanosim_amd/csrc/ns_pack.h"

// a = column (-1: the first-match column) | previous match | error type | Markov state; u, u2 = draws
enum : int { LP_GV = 0,        // ecdf_lookup_gv on the full one-word column `a`                 (a, u)
             LP_NEXT = 1,      // next_match_gv behind the previous match `a`                    (a, u)
             LP_G64 = 2,       // ecdf_lookup_g<double> on the fp64 column `a`                   (a, u)
             LP_RUN_R = 3,     // run_length_r of error type `a`                                 (a, u = u_mix, u2 = u_len)
             LP_RUN_T = 4,     // run_length_t of error type `a`
             LP_TRANS = 5,     // trans_pick_u on the packed row of state `a`                    (a, u)
             LP_N = 6 };

template <int OP> NS_DEV int32_t lp_one(const Tabs &T, const Tabs &TG, const ChainTab &c, int32_t a, uint32_t u, uint32_t u2) {
    if (OP == LP_GV || OP == LP_G64) {
        if (a < 0) {
            if (OP == LP_GV) return ecdf_lookup_gv(TG.q(c.fm_gv), c.fm_n, T.h(c.fm_guide), u, TG.q(c.sub2_full), TG.d(c.fm_hi), TG.d(c.fm_vhi), c.fm_vlo0);
            return ecdf_lookup_g(TG.d(c.fm_hi), TG.d(c.fm_vhi), c.fm_n, c.fm_vlo0, TG.h(c.fm_guide), u);
        }
        const uint32_t b = (uint32_t)a, o = T.u(c.mm_seg_off)[b], nc = T.u(c.mm_seg_off)[b + 1] - o;
        if (OP == LP_GV)
            return ecdf_lookup_gv(TG.q(c.mm_gv_full) + o, nc, T.h(c.mm_guide) + NS_GUIDE_CELLS * b, u, TG.q(c.sub2_full), TG.d(c.mm_hi) + o, TG.d(c.mm_vhi) + o, T.d(c.mm_vlo0)[b]);
        return ecdf_lookup_g(TG.d(c.mm_hi) + o, TG.d(c.mm_vhi) + o, nc, TG.d(c.mm_vlo0)[b], TG.h(c.mm_guide) + NS_GUIDE_CELLS * b, u);
    }
    if (OP == LP_NEXT) return next_match_gv(T, TG, c, a, u);
    if (OP == LP_RUN_R) return run_length_r(T, c, (uint32_t)a, T.q(c.mix_w)[a], u, u2);
    if (OP == LP_RUN_T) return run_length_t(T, c, a, u, u2);
    return trans_pick_u(T.q(c.trans) + 3 * a, u);
}

struct Probe {
    ChainTab ct;
    std::vector<uint64_t> blob, lds;          // lds: a copy of the first n_words_lds words
    bool whole;
    uint64_t *d_blob = nullptr, *d_lds = nullptr;
};

// is `a` an index the look-up may take?  (the draws are free: every 32-bit value is a draw)
static bool lp_valid(const Probe *h, int op, const int32_t *a, uint64_t n) {
    int32_t lo = 0, hi = 0x7fffffff;
    if (op == LP_GV || op == LP_G64) { lo = -1; hi = (int32_t)h->ct.mm_nbins - 1; }
    if (op == LP_RUN_R || op == LP_RUN_T) hi = 2;
    if (op == LP_TRANS) hi = 6;
    for (uint64_t i = 0; i < n; ++i) if (a[i] < lo || a[i] > hi) return false;
    return true;
}

#ifdef NS_HOST_TEST
template <int OP> static void lp_run(const Probe *h, const int32_t *a, const uint32_t *u, const uint32_t *u2, int32_t *out, uint64_t n) {
    const Tabs T{h->lds.data()}, TG{h->blob.data()};
    for (uint64_t i = 0; i < n; ++i) out[i] = lp_one<OP>(T, TG, h->ct, a[i], u[i], u2[i]);
}
static int lp_upload(Probe *) { return 0; }
static void lp_release(Probe *) {}
#else
// the LDS part is copied into LDS while it fits next to nothing else (k_chain<LDS> does so up to 44 KB); every thread checks its index
#define LP_LDS_MAX_BYTES (60u * 1024u)
template <int OP, bool LDS> __global__ void __launch_bounds__(256) k_lp(const uint64_t *__restrict__ blob, const uint64_t *__restrict__ lds_part, ChainTab c,
                                                                        const int32_t *__restrict__ a, const uint32_t *__restrict__ u,
                                                                        const uint32_t *__restrict__ u2, int32_t *__restrict__ out, uint64_t n) {
    extern __shared__ uint64_t lp_image[];
    const uint64_t *tw = lds_part;
    if (LDS) {
        for (uint32_t i = threadIdx.x; i < c.n_words_lds; i += blockDim.x) lp_image[i] = lds_part[i];
        __syncthreads();
        tw = lp_image;
    }
    const Tabs T{tw}, TG{blob};
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) out[i] = lp_one<OP>(T, TG, c, a[i], u[i], u2[i]);
}
template <int OP> static void lp_launch(const Probe *h, const int32_t *a, const uint32_t *u, const uint32_t *u2, int32_t *out, uint64_t n) {
    const uint64_t nb = (n + 255) / 256;
    const uint32_t grid = (uint32_t)(nb < 1024 ? (nb ? nb : 1) : 1024);
    const size_t bytes = (size_t)h->ct.n_words_lds * 8;
    if (bytes <= LP_LDS_MAX_BYTES) k_lp<OP, true><<<grid, 256, bytes>>>(h->d_blob, h->d_lds, h->ct, a, u, u2, out, n);
    else k_lp<OP, false><<<grid, 256, 0>>>(h->d_blob, h->d_lds, h->ct, a, u, u2, out, n);
}
static int lp_upload(Probe *h) {
    hipError_t e = hipMalloc(&h->d_blob, h->blob.size() * 8);
    if (e == hipSuccess) e = hipMalloc(&h->d_lds, h->lds.size() * 8 + 8);
    if (e == hipSuccess) e = hipMemcpy(h->d_blob, h->blob.data(), h->blob.size() * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(h->d_lds, h->lds.data(), h->lds.size() * 8, hipMemcpyHostToDevice);
    return (int)e;
}
static void lp_release(Probe *h) { if (h->d_blob) (void)hipFree(h->d_blob); if (h->d_lds) (void)hipFree(h->d_lds); }
#endif

extern "C" {

#ifdef NS_HOST_TEST
int lp_gpu(void) { return 0; }
#else
int lp_gpu(void) { return 1; }
#endif
uint32_t lp_cells(void) { return NS_GUIDE_CELLS; }
uint32_t lp_cell_start(uint32_t cell) { return guide_cell_start(cell); }
uint32_t lp_ct_size(void) { return (uint32_t)sizeof(ChainTab); }

void lp_free(void *p) {
    Probe *h = static_cast<Probe *>(p);
    if (h) { lp_release(h); delete h; }
}
void *lp_pack(const ns_model_tables *t, uint32_t force_tail_bits) {
    Probe *h = new (std::nothrow) Probe;
    if (!h) return nullptr;
    ns_pack_chain_tables(t, t->mm_seg_off[t->mm_nbins], h->ct, h->blob, h->whole, force_tail_bits);
    h->lds.assign(h->blob.begin(), h->blob.begin() + h->ct.n_words_lds);
    if (lp_upload(h) != 0) { lp_free(h); return nullptr; }
    return h;
}
int lp_whole(const void *p) { return static_cast<const Probe *>(p)->whole ? 1 : 0; }
void lp_ct(const void *p, void *out) { memcpy(out, &static_cast<const Probe *>(p)->ct, sizeof(ChainTab)); }
const uint64_t *lp_blob(const void *p) { return static_cast<const Probe *>(p)->blob.data(); }

// out[i] = look-up `op` of (a[i], u[i], u2[i]).  Returns 0; -1 unknown op; -2 an index out of range; -3 the integer image is not valid for
// this model (value edges that are no whole numbers: LP_GV and LP_NEXT are not what the engine runs then); a HIP error code otherwise.
int lp_eval(const void *p, int op, const int32_t *a, const uint32_t *u, const uint32_t *u2, int32_t *out, uint64_t n) {
    const Probe *h = static_cast<const Probe *>(p);
    if (op < 0 || op >= LP_N) return -1;
    if (!lp_valid(h, op, a, n)) return -2;
    if ((op == LP_GV || op == LP_NEXT) && !h->whole) return -3;
    if (!n) return 0;
#ifdef NS_HOST_TEST
    switch (op) {
    case LP_GV: lp_run<LP_GV>(h, a, u, u2, out, n); break;       case LP_NEXT: lp_run<LP_NEXT>(h, a, u, u2, out, n); break;
    case LP_G64: lp_run<LP_G64>(h, a, u, u2, out, n); break;     case LP_RUN_R: lp_run<LP_RUN_R>(h, a, u, u2, out, n); break;
    case LP_RUN_T: lp_run<LP_RUN_T>(h, a, u, u2, out, n); break; case LP_TRANS: lp_run<LP_TRANS>(h, a, u, u2, out, n); break;
    }
    return 0;
#else
    void *d[4] = {nullptr, nullptr, nullptr, nullptr};
    const void *src[3] = {a, u, u2};
    hipError_t e = hipSuccess;
    for (int k = 0; k < 4 && e == hipSuccess; ++k) {
        e = hipMalloc(&d[k], n * 4);
        if (e == hipSuccess && k < 3) e = hipMemcpy(d[k], src[k], n * 4, hipMemcpyHostToDevice);
    }
    if (e == hipSuccess) {
        const int32_t *da = static_cast<const int32_t *>(d[0]);
        const uint32_t *du = static_cast<const uint32_t *>(d[1]), *du2 = static_cast<const uint32_t *>(d[2]);
        int32_t *dout = static_cast<int32_t *>(d[3]);
        switch (op) {
        case LP_GV: lp_launch<LP_GV>(h, da, du, du2, dout, n); break;       case LP_NEXT: lp_launch<LP_NEXT>(h, da, du, du2, dout, n); break;
        case LP_G64: lp_launch<LP_G64>(h, da, du, du2, dout, n); break;     case LP_RUN_R: lp_launch<LP_RUN_R>(h, da, du, du2, dout, n); break;
        case LP_RUN_T: lp_launch<LP_RUN_T>(h, da, du, du2, dout, n); break; case LP_TRANS: lp_launch<LP_TRANS>(h, da, du, du2, dout, n); break;
        }
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, d[3], n * 4, hipMemcpyDeviceToHost);
    for (int k = 0; k < 4; ++k) if (d[k]) (void)hipFree(d[k]);
    return (int)e;
#endif
}

}  // extern "C"
