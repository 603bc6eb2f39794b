// math_probe.hip — TEST infrastructure: the engine's scalar primitives (nanosim_amd/csrc/ns_rng.h, ns_device.h) evaluated over arrays of
// inputs, so that tests/test_math_probe.py can hold them against the oracle's copies (oracle/ns_oracle.c nso_eval_batch) bit for bit.
// Built by the test twice, into a temporary directory:
//   for gfx950:    hipcc <the engine's HIP_FLAGS>                                   one bounds-checked kernel per primitive
//   for the host:  hipcc --cuda-host-only -x hip -O3 -std=c++17 -ffp-contract=off -DNS_HOST_TEST -shared -fPIC   the same functions in a loop
// Nothing of the product links or loads this file.
#include <new>
#include "../nanosim_amd/csrc/ns_device.h"
#include "../nanosim_amd/csrc/ns_hp.h"        // (include order of the engine: ns_hp.h pulls in ns_materialise.h)

// the op numbers of nso_eval_batch; in / out are 8-byte elements (double, or uint64 for the draw ops)
enum : int { OP_LOG = 0, OP_EXP = 1, OP_NORMINV_U = 2, OP_POW10M1 = 3, OP_U53 = 4, OP_THR_LT = 5, OP_THR_GT = 6, OP_F64_I64 = 7,
             OP_NORMINV = 8, OP_LEN_DRAW = 9, OP_N = 10 };

template <int OP> NS_HD void eval_one(const uint64_t *in, uint64_t *out, uint64_t i) {
    const uint64_t x = in[i];
    const double d = ns_bits_to_double(x);
    if (OP == OP_LOG) out[i] = ns_double_to_bits(ns_log(d));
    if (OP == OP_EXP) out[i] = ns_double_to_bits(ns_exp(d));
    if (OP == OP_NORMINV_U) out[i] = ns_double_to_bits(ns_norminv(u32_to_p((uint32_t)x)));
    if (OP == OP_POW10M1) out[i] = ns_double_to_bits(ns_pow10m1(d));
    if (OP == OP_U53) out[i] = ns_double_to_bits(u53_to_p((uint32_t)(x >> 32), (uint32_t)x));
    if (OP == OP_THR_LT) out[i] = ns_thr_lt(d);
    if (OP == OP_THR_GT) out[i] = ns_thr_gt(d);
    if (OP == OP_F64_I64) out[i] = (uint64_t)ns_f64_to_i64_sat(d);
    if (OP == OP_NORMINV) out[i] = ns_double_to_bits(ns_norminv(d));
    if (OP == OP_LEN_DRAW) out[i] = (uint64_t)ns_len_draw(d);
}

#ifdef NS_HOST_TEST
// ---- host build: the same functions, in a loop -------------------------------------------------------------------------------------
template <int OP> static void run(const uint64_t *in, uint64_t *out, uint64_t n) { for (uint64_t i = 0; i < n; ++i) eval_one<OP>(in, out, i); }

extern "C" {
int probe_gpu(void) { return 0; }
int probe_eval(int op, const void *in, void *out, uint64_t n) {
    const uint64_t *x = static_cast<const uint64_t *>(in);
    uint64_t *y = static_cast<uint64_t *>(out);
    switch (op) {
    case OP_LOG: run<OP_LOG>(x, y, n); break;             case OP_EXP: run<OP_EXP>(x, y, n); break;
    case OP_NORMINV_U: run<OP_NORMINV_U>(x, y, n); break; case OP_POW10M1: run<OP_POW10M1>(x, y, n); break;
    case OP_U53: run<OP_U53>(x, y, n); break;             case OP_THR_LT: run<OP_THR_LT>(x, y, n); break;
    case OP_THR_GT: run<OP_THR_GT>(x, y, n); break;       case OP_F64_I64: run<OP_F64_I64>(x, y, n); break;
    case OP_NORMINV: run<OP_NORMINV>(x, y, n); break;     case OP_LEN_DRAW: run<OP_LEN_DRAW>(x, y, n); break;
    default: return -1;
    }
    return 0;
}
int probe_ecdf(const double *hi, const double *vhi, uint32_t nseg, double vlo0, const double *p, int64_t *out, uint64_t n) {
    for (uint64_t i = 0; i < n; ++i) out[i] = ecdf_lookup(hi, vhi, nseg, vlo0, p[i]);
    return 0;
}
int probe_table_value(const double *cdf, uint32_t nc, const double *p, int64_t *out, uint64_t n) {
    for (uint64_t i = 0; i < n; ++i) out[i] = table_value(cdf, nc, p[i]);
    return 0;
}
int probe_trans_pick(const uint64_t *row, const uint32_t *u, int32_t *out, uint64_t n) {
    for (uint64_t i = 0; i < n; ++i) out[i] = trans_pick_u(row, u[i]);
    return 0;
}
}  // extern "C"

#else
// ---- gfx950 build: one kernel per primitive, every thread checks its index ----------------------------------------------------------
template <int OP> __global__ void __launch_bounds__(256) k_eval(const uint64_t *__restrict__ in, uint64_t *__restrict__ out, uint64_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) eval_one<OP>(in, out, i);
}
__global__ void __launch_bounds__(256) k_ecdf(const double *hi, const double *vhi, uint32_t nseg, double vlo0, const double *p, int64_t *out, uint64_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) out[i] = ecdf_lookup(hi, vhi, nseg, vlo0, p[i]);
}
__global__ void __launch_bounds__(256) k_table_value(const double *cdf, uint32_t nc, const double *p, int64_t *out, uint64_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) out[i] = table_value(cdf, nc, p[i]);
}
__global__ void __launch_bounds__(256) k_trans_pick(const uint64_t *row, const uint32_t *u, int32_t *out, uint64_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) out[i] = trans_pick_u(row, u[i]);
}
// norminv(u32_to_p(u)) non-decreasing over every u: thread t walks u in [256 t, 256 t + 256] (one past its block: the boundaries overlap)
__global__ void __launch_bounds__(256) k_norminv_monotone(unsigned long long *bad, unsigned long long *first_bad) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (1ull << 24)) return;
    const uint64_t u0 = t << 8;
    double prev = ns_norminv(u32_to_p((uint32_t)u0));
    for (uint64_t u = u0 + 1; u <= u0 + 256 && u <= 0xffffffffull; ++u) {
        const double v = ns_norminv(u32_to_p((uint32_t)u));
        if (v < prev) { atomicAdd(bad, 1ull); atomicMin(first_bad, (unsigned long long)u); }
        prev = v;
    }
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

template <int OP> static void launch(const uint64_t *in, uint64_t *out, uint64_t n) { k_eval<OP><<<grid_for(n), 256>>>(in, out, n); }

extern "C" {
int probe_gpu(void) { return 1; }
int probe_eval(int op, const void *in, void *out, uint64_t n) {
    if (op < 0 || op >= OP_N) return -1;
    DevBufs b;
    const uint64_t *x = static_cast<const uint64_t *>(b.get(in, n * 8));
    uint64_t *y = static_cast<uint64_t *>(b.get(nullptr, n * 8));
    if (b.err == hipSuccess && n) {
        switch (op) {
        case OP_LOG: launch<OP_LOG>(x, y, n); break;             case OP_EXP: launch<OP_EXP>(x, y, n); break;
        case OP_NORMINV_U: launch<OP_NORMINV_U>(x, y, n); break; case OP_POW10M1: launch<OP_POW10M1>(x, y, n); break;
        case OP_U53: launch<OP_U53>(x, y, n); break;             case OP_THR_LT: launch<OP_THR_LT>(x, y, n); break;
        case OP_THR_GT: launch<OP_THR_GT>(x, y, n); break;       case OP_F64_I64: launch<OP_F64_I64>(x, y, n); break;
        case OP_NORMINV: launch<OP_NORMINV>(x, y, n); break;     case OP_LEN_DRAW: launch<OP_LEN_DRAW>(x, y, n); break;
        }
    }
    return b.finish(out, y, n * 8);
}
int probe_ecdf(const double *hi, const double *vhi, uint32_t nseg, double vlo0, const double *p, int64_t *out, uint64_t n) {
    if (nseg == 0) return -1;
    DevBufs b;
    const double *dh = static_cast<const double *>(b.get(hi, nseg * 8ull)), *dv = static_cast<const double *>(b.get(vhi, nseg * 8ull));
    const double *dp = static_cast<const double *>(b.get(p, n * 8));
    int64_t *dout = static_cast<int64_t *>(b.get(nullptr, n * 8));
    if (b.err == hipSuccess && n) k_ecdf<<<grid_for(n), 256>>>(dh, dv, nseg, vlo0, dp, dout, n);
    return b.finish(out, dout, n * 8);
}
int probe_table_value(const double *cdf, uint32_t nc, const double *p, int64_t *out, uint64_t n) {
    if (nc == 0) return -1;
    DevBufs b;
    const double *dc = static_cast<const double *>(b.get(cdf, nc * 8ull)), *dp = static_cast<const double *>(b.get(p, n * 8));
    int64_t *dout = static_cast<int64_t *>(b.get(nullptr, n * 8));
    if (b.err == hipSuccess && n) k_table_value<<<grid_for(n), 256>>>(dc, nc, dp, dout, n);
    return b.finish(out, dout, n * 8);
}
int probe_trans_pick(const uint64_t *row, const uint32_t *u, int32_t *out, uint64_t n) {
    DevBufs b;
    const uint64_t *dr = static_cast<const uint64_t *>(b.get(row, 2 * 8));
    const uint32_t *du = static_cast<const uint32_t *>(b.get(u, n * 4));
    int32_t *dout = static_cast<int32_t *>(b.get(nullptr, n * 4));
    if (b.err == hipSuccess && n) k_trans_pick<<<grid_for(n), 256>>>(dr, du, dout, n);
    return b.finish(out, dout, n * 4);
}
// counts the u in [1, 2^32) with norminv(p(u)) < norminv(p(u - 1)); *first_bad: the least of them (~0 if none)
int probe_norminv_monotone(uint64_t *n_bad, uint64_t *first_bad) {
    DevBufs b;
    const unsigned long long init[2] = {0ull, ~0ull};
    unsigned long long *d = static_cast<unsigned long long *>(b.get(init, sizeof init));
    if (b.err == hipSuccess) k_norminv_monotone<<<(1u << 24) / 256, 256>>>(d, d + 1);
    unsigned long long res[2] = {0ull, 0ull};
    const int rc = b.finish(res, d, sizeof res);
    *n_bad = res[0]; *first_bad = res[1];
    return rc;
}
}  // extern "C"
#endif
