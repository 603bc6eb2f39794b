// qual_probe.hip — TEST infrastructure: the engine's base-quality look-ups (nanosim_amd/csrc/ns_device.h qual_value, qual_value_lut;
// ns_materialise.h qual_lookup16) and the bucket-table builder of ns_load_model (ns_pack.h ns_build_qual_lut) evaluated directly, so that
// tests/test_qual_probe.py can hold them against the exact count q = #{j < 127 : h >= thr[j]} over every 16-bit draw h.
// Built by the test twice, into a temporary directory, as tests/math_probe.hip:
//   for gfx950:    hipcc <the engine's HIP_FLAGS>                                   bounds-checked kernels, and qual_lookup16 as k_qualities runs it
//   for the host:  hipcc --cuda-host-only -x hip -O3 -std=c++17 -ffp-contract=off -DNS_HOST_TEST -shared -fPIC   qual_value, qual_value_lut in a loop
// Nothing of the product links or loads this file.
#include <new>
#include "../nanosim_amd/csrc/ns_materialise.h"
#include "../nanosim_amd/csrc/ns_pack.h"

extern "C" {
// one class: thr[NS_QUAL_LEVELS] -> lut[1024], the builder of ns_load_model (host code in both builds)
int probe_build_lut(const uint32_t *thr, uint16_t *lut) { ns_build_qual_lut(thr, lut); return 0; }
uint32_t probe_thr_decrease(const uint32_t *thr) { return ns_qual_thr_decrease(thr); }
}

#ifdef NS_HOST_TEST
// ---- host build: the same functions, in a loop -------------------------------------------------------------------------------------
extern "C" {
int probe_gpu(void) { return 0; }
int probe_qual_value(const uint32_t *thr, const uint32_t *h, uint8_t *out, uint64_t n) {
    for (uint64_t i = 0; i < n; ++i) out[i] = qual_value(thr, h[i]);
    return 0;
}
int probe_qual_value_lut(const uint32_t *thr, const uint16_t *lut, const uint32_t *h, uint8_t *out, uint64_t n) {
    for (uint64_t i = 0; i < n; ++i) out[i] = qual_value_lut(thr, lut, h[i]);
    return 0;
}
}  // extern "C"

#else
// ---- gfx950 build ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_qual_value(const uint32_t *thr, const uint32_t *h, uint8_t *out, uint64_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) out[i] = qual_value(thr, h[i]);
}
__global__ void __launch_bounds__(256) k_qual_value_lut(const uint32_t *thr, const uint16_t *lut, const uint32_t *h, uint8_t *out, uint64_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        out[i] = qual_value_lut(thr, lut, h[i]);
}
// qual_lookup16 as k_qualities runs it: one workgroup = one wavefront, the bucket tables of all classes in LDS (qual_lut_load), 16 draws
// per lane.  Lane t of wave w: draws D[8] at D + 8 (64 w + t) (position i: halfword i & 1 of D[i >> 1]), classes cls[16] at cls + 16 (64 w + t),
// its 16 qualities at out + 16 (64 w + t).  A lane of classes in {match, substituted, inserted} takes its class words the way the record
// kernel leaves them (class bits on record bytes -> cls_pack16 -> cls_unpack4); a lane whose first class is ht or unmapped takes the
// constant words of qualities_head_tail / a gap piece (its 16 classes are all that one).
__global__ void __launch_bounds__(64) k_lookup16(DevModel m, const uint32_t *__restrict__ D, const uint8_t *__restrict__ cls, uint8_t *__restrict__ out,
                                                 uint32_t nwaves) {
    __shared__ __align__(16) uint16_t qlut[NS_QLUT_SLOTS * 1024u];
    qual_lut_load(qlut, m, threadIdx.x, 64);
    __syncthreads();
    if (blockIdx.x >= nwaves || threadIdx.x >= 64) return;
    const uint64_t l = (uint64_t)blockIdx.x * 64u + threadIdx.x;
    uint32_t d[8], cs[4];
    for (uint32_t k = 0; k < 8; ++k) d[k] = D[8 * l + k];
    const uint8_t *c = cls + 16 * l;
    if (c[0] >= (uint8_t)NS_Q_HT) {
        cs[0] = cs[1] = cs[2] = cs[3] = 0x08080808u * (uint32_t)c[0];
    } else {
        uint32_t r[4];
        for (uint32_t k = 0; k < 4; ++k) {
            r[k] = 0;
            for (uint32_t i = 0; i < 4; ++i) {
                const uint32_t ci = c[4 * k + i];
                const uint32_t b = 'A' | (ci == NS_Q_MIS ? NS_CLS_MIS_BIT : ci == NS_Q_INS ? NS_CLS_INS_BIT : 0u);
                r[k] |= b << (8 * i);
            }
        }
        const uint32_t w = cls_pack16(r[0], r[1], r[2], r[3]);
        for (uint32_t k = 0; k < 4; ++k) cs[k] = cls_unpack4(w, k);
    }
    QualState Q; Q.lut = qlut;
    uint64_t qlo, qhi;
    qual_lookup16(Q, m, d, cs, qlo, qhi);
    uint64_t *o = reinterpret_cast<uint64_t *>(out + 16 * l);
    o[0] = qlo; o[1] = qhi;
}

static uint32_t grid_for(uint64_t n) { const uint64_t b = (n + 255) / 256; return (uint32_t)(b < 65536 ? (b ? b : 1) : 65536); }

// device buffers of one call, freed on every path
struct DevBufs {
    void *p[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    int k = 0;
    hipError_t err = hipSuccess;
    void *get(const void *host, size_t bytes) {
        void *d = nullptr;
        if (err != hipSuccess) return nullptr;
        err = hipMalloc(&d, bytes ? bytes : 8);
        if (err != hipSuccess) return nullptr;
        p[k++] = d;
        if (host && bytes) err = hipMemcpy(d, host, bytes, hipMemcpyHostToDevice);
        return d;
    }
    int finish(void *host, const void *dev, size_t bytes) {
        if (err == hipSuccess) err = hipGetLastError();
        if (err == hipSuccess) err = hipDeviceSynchronize();
        if (err == hipSuccess && bytes) err = hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost);
        for (int i = 0; i < k; ++i) (void)hipFree(p[i]);
        return (int)err;
    }
};

extern "C" {
int probe_gpu(void) { return 1; }
int probe_qual_value(const uint32_t *thr, const uint32_t *h, uint8_t *out, uint64_t n) {
    DevBufs b;
    const uint32_t *dt = static_cast<const uint32_t *>(b.get(thr, NS_QUAL_LEVELS * 4)), *dh = static_cast<const uint32_t *>(b.get(h, n * 4));
    uint8_t *dout = static_cast<uint8_t *>(b.get(nullptr, n));
    if (b.err == hipSuccess && n) k_qual_value<<<grid_for(n), 256>>>(dt, dh, dout, n);
    return b.finish(out, dout, n);
}
int probe_qual_value_lut(const uint32_t *thr, const uint16_t *lut, const uint32_t *h, uint8_t *out, uint64_t n) {
    DevBufs b;
    const uint32_t *dt = static_cast<const uint32_t *>(b.get(thr, NS_QUAL_LEVELS * 4));
    const uint16_t *dl = static_cast<const uint16_t *>(b.get(lut, 1024 * 2));
    const uint32_t *dh = static_cast<const uint32_t *>(b.get(h, n * 4));
    uint8_t *dout = static_cast<uint8_t *>(b.get(nullptr, n));
    if (b.err == hipSuccess && n) k_qual_value_lut<<<grid_for(n), 256>>>(dt, dl, dh, dout, n);
    return b.finish(out, dout, n);
}
// thr: [NS_Q_COUNT][NS_QUAL_LEVELS], lut: [NS_Q_COUNT][1024] (the slots qual_lut_load copies), D: nwaves * 64 * 8 words, cls and out:
// nwaves * 64 * 16 bytes
int probe_lookup16(const uint32_t *thr, const uint16_t *lut, const uint32_t *D, const uint8_t *cls, uint8_t *out, uint32_t nwaves) {
    DevBufs b;
    const size_t lanes = (size_t)nwaves * 64u;
    DevModel m;
    memset(&m, 0, sizeof m);
    m.qual_thr = static_cast<const uint32_t *>(b.get(thr, (size_t)NS_Q_COUNT * NS_QUAL_LEVELS * 4));
    m.qual_lut = static_cast<const uint16_t *>(b.get(lut, (size_t)NS_QLUT_SLOTS * 1024 * 2));
    const uint32_t *dD = static_cast<const uint32_t *>(b.get(D, lanes * 32));
    const uint8_t *dc = static_cast<const uint8_t *>(b.get(cls, lanes * 16));
    uint8_t *dout = static_cast<uint8_t *>(b.get(nullptr, lanes * 16));
    if (b.err == hipSuccess && nwaves) k_lookup16<<<nwaves, 64>>>(m, dD, dc, dout, nwaves);
    return b.finish(out, dout, lanes * 16);
}
}  // extern "C"
#endif
