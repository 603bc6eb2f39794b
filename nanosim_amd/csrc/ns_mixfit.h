// ns_mixfit.h — training side, the error-length mixtures: what src/model_fitting.py fits to the three length histograms —
// the Poisson-geometric mixture of mismatch runs (mis_ll / mis_fit, F:48-65) and the Weibull-geometric mixtures of insertion and deletion
// runs (ins_ll / ins_fit, del_ll / del_fit, F:68-105) — as ONE search per start: the objective, and scipy's Nelder-Mead around it.
// F: = src/model_fitting.py, M: = src/mixed_model.py of bcgsc/NanoSim v3.2.2; scipy 1.15 (stats/_distn_infrastructure.py: rv_discrete.cdf,
// optimize/_optimize.py: _minimize_neldermead).
// The code below compiles for the device (k_mixfit, ns_train.h: one wavefront per start, a lane per bin of a tile) and, unchanged, for the
// host (tests/mixfit_host.cpp: one thread walks the 64 lanes as a 64-entry array).  MF_W is the number of lanes a thread stands for.
//
// THE OBJECTIVES.  cdf[0 .. n) is the empirical CDF (read_histogram, F:27-45).
//  * mismatch, parameters (l, p, w), bin x = 0 .. n-1 (F:55; M:15-18; rv_discrete without _cdf sums _pmf from a = 0):
//        pmf(x) = w * exp(x * log l - ln x! - l) + (1 - w) * p * (1 - p)^x,   C(x) = pmf(0) + ... + pmf(x)
//  * insertion / deletion, parameters (l, k, p, w), bin j = 0 .. n-1 stands for x = j + 1 (F:76; M:21-25; geom with loc = -1):
//        C(x) = w * (1 - exp(-(x / l)^k)) + (1 - w) * (1 - (1 - p)^(x + 1))
//  * value: the largest |clip(C, 0, 1) - cdf| over the bins (rv_discrete.cdf clips; the sum itself is not clipped, so w > 1 can carry it
//    below 0 and back).
//  * THE NaN RULE: a parameter that is not > 0 fails rv_discrete's default _argcheck, p > 1 fails geom's own; either makes every CDF value
//    NaN and the objective is NaN (mf_nan(): one bit pattern).  No other input makes a NaN: every term below is finite for finite parameters.
//  * arithmetic: + - * /, ns_log and ns_exp (ns_rng.h) only, powers as ns_exp(k * ns_log(.)), no fused multiply-add outside those two (the
//    builds use -ffp-contract=off), ln x! from a table the host passes in (mf_lnfact_table).  ns_exp clamps its argument to +-700, so
//    (1 - p)^x for p = 1 (ns_log(0) = -1023 ln 2) and exp(-(x / l)^k) for a power beyond the range come out as 1e-304, not as 0: far
//    below the 1e-12 the values are held to.
// THE EVALUATION ORDER, which both builds follow so that they return the same 64 bits:
//  * bins in tiles of 64, lane j of tile t has bin 64 t + j; lanes beyond n hold 0 and take no part in the maximum;
//  * mismatch: a six-step inclusive scan inside the tile — for d = 1, 2, 4, 8, 16, 32: v[j] += v[j - d] for j >= d, all j at once —,
//    then C = carry + v[j], and carry = carry + v[63] for the next tile (carry starts at 0);
//  * the maximum: per lane over its tiles in ascending order (m = d > m ? d : m, m starts at 0), then over the 64 lanes.  The values are
//    no NaN and no -0, so the maximum of the lanes does not depend on the order; the device takes the xor butterfly 32, 16, .. 1.
//
// THE SEARCH: _minimize_neldermead as minimize(f, x0, method='Nelder-Mead') runs it — initial simplex x0 and x0 with one coordinate times
// 1.05 (0.00025 for a zero), rho chi psi sigma = 1 2 0.5 0.5 written out as the products scipy forms, xatol = fatol = 1e-4,
// maxiter = maxfev = 200 N, an evaluation refused at the limit ends the iteration where it stands (a shrink has then moved a vertex
// whose value is stale: scipy's does), every sort in np.argsort's order (MfSimplex::sort), fun = np.min(fsim), which is NaN as soon as one
// vertex is.  The simplex lives in registers: every index below is a compile-time constant after unrolling.
#pragma once
#include <stdint.h>
#include <math.h>
#include "ns_rng.h"
#include "../../include/nanosim_amd.h"

#define MF_TILE 64u
#define MF_MAX_BINS 65536u
#if defined(__HIP_DEVICE_COMPILE__)
#define MF_W 1u
#else
#define MF_W 64u
#endif

NS_HD double mf_nan() { return ns_bits_to_double(0x7ff8000000000000ull); }
NS_HD double mf_exp(double t) { return ns_exp(t == t ? t : 0.0); }          // (ns_exp converts its argument to an integer: never a NaN)
NS_HD double mf_clip01(double c) { c = c < 0.0 ? 0.0 : c; return c > 1.0 ? 1.0 : c; }
NS_HD double mf_absdiff(double a, double b) { const double d = a - b; return d < 0.0 ? -d : d; }

// the lane that entry i of a thread's MF_W values stands for
NS_HD uint32_t mf_lane(uint32_t i) {
#if defined(__HIP_DEVICE_COMPILE__)
    (void)i; return threadIdx.x & 63u;
#else
    return i;
#endif
}
// the inclusive scan over the 64 lanes of a tile, in the order written above
NS_HD void mf_tile_scan(double (&v)[MF_W]) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (uint32_t d = 1; d < MF_TILE; d <<= 1) { const double u = __shfl_up(v[0], d, 64); if (lane >= d) v[0] += u; }
#else
    for (uint32_t d = 1; d < MF_TILE; d <<= 1) for (uint32_t j = MF_TILE - 1u; j >= d; --j) v[j] += v[j - d];
#endif
}
NS_HD double mf_tile_last(const double (&v)[MF_W]) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __shfl(v[0], 63, 64);
#else
    return v[MF_TILE - 1u];
#endif
}
NS_HD double mf_lane_max(const double (&m)[MF_W]) {
#if defined(__HIP_DEVICE_COMPILE__)
    double r = m[0];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const double u = __shfl_xor(r, o, 64); r = u > r ? u : r; }
    return r;
#else
    double r = m[0];
    for (uint32_t j = 1; j < MF_TILE; ++j) r = m[j] > r ? m[j] : r;
    return r;
#endif
}

// ln x! for x = 0 .. n-1: the table both builds read, made on the host (its lgamma; gammaln(x + 1) in the reference)
static inline void mf_lnfact_table(double *t, uint32_t n) { for (uint32_t x = 0; x < n; ++x) t[x] = x < 2u ? 0.0 : lgamma((double)x + 1.0); }

// mismatch: x = (l, p, w)
struct MfMis {
    static constexpr int N = 3;
    const double *cdf, *lnf; uint32_t n;
    NS_HD double operator()(const double (&x)[4]) const {
        const double l = x[0], p = x[1], w = x[2];
        if (!(l > 0.0) || !(p > 0.0) || !(w > 0.0) || p > 1.0) return mf_nan();
        const double ll = ns_log(l), lq = ns_log(1.0 - p), w1 = 1.0 - w;
        double carry = 0.0, m[MF_W], v[MF_W];
        for (uint32_t i = 0; i < MF_W; ++i) m[i] = 0.0;
        for (uint32_t base = 0; base < n; base += MF_TILE) {
            for (uint32_t i = 0; i < MF_W; ++i) {
                const uint32_t bin = base + mf_lane(i);
                v[i] = 0.0;
                if (bin < n) {
                    const double xd = (double)bin;
                    const double pois = mf_exp((xd * ll - lnf[bin]) - l), geo = p * mf_exp(xd * lq);
                    v[i] = w * pois + w1 * geo;
                }
            }
            mf_tile_scan(v);
            for (uint32_t i = 0; i < MF_W; ++i) {
                const uint32_t bin = base + mf_lane(i);
                if (bin < n) { const double d = mf_absdiff(mf_clip01(carry + v[i]), cdf[bin]); m[i] = d > m[i] ? d : m[i]; }
            }
            carry = carry + mf_tile_last(v);
        }
        return mf_lane_max(m);
    }
};
// insertion / deletion: x = (l, k, p, w)
struct MfIndel {
    static constexpr int N = 4;
    const double *cdf, *lnf; uint32_t n;              // (lnf is not read)
    NS_HD double operator()(const double (&x)[4]) const {
        const double l = x[0], k = x[1], p = x[2], w = x[3];
        if (!(l > 0.0) || !(k > 0.0) || !(p > 0.0) || !(w > 0.0) || p > 1.0) return mf_nan();
        const double lq = ns_log(1.0 - p), w1 = 1.0 - w;
        double m[MF_W];
        for (uint32_t i = 0; i < MF_W; ++i) m[i] = 0.0;
        for (uint32_t base = 0; base < n; base += MF_TILE)
            for (uint32_t i = 0; i < MF_W; ++i) {
                const uint32_t bin = base + mf_lane(i);
                if (bin < n) {
                    const double xd = (double)bin + 1.0;
                    const double wei = 1.0 - mf_exp(-mf_exp(k * ns_log(xd / l))), geo = 1.0 - mf_exp((xd + 1.0) * lq);
                    const double d = mf_absdiff(mf_clip01(w * wei + w1 * geo), cdf[bin]);
                    m[i] = d > m[i] ? d : m[i];
                }
            }
        return mf_lane_max(m);
    }
};

// np.argsort's order of two values: a before b
NS_HD bool mf_less(double a, double b) { return a < b || (b != b && a == a); }

// THE ORDER OF THE SIMPLEX is the order np.argsort gives scipy on the N + 1 values, ties included — the objective is a maximum over a
// few bins and takes the same value at different points often enough (a clipped CDF against the same bin) that searches part ways there:
//  * with a NaN among the values numpy falls back to std::sort with "NaN last": an insertion sort below 17 values, stable;
//  * without one, numpy 2 sorts float64 indices with x86-simd-sort on AVX-512 hardware (where the reference's fixture was made): the values
//    in the low lanes of an 8-lane register, +inf in the rest, through the six compare-exchange stages of a bitonic sort — partner
//    i^1, reverse within 4, i^1, 7-i, i^2, i^1; the higher lane of a pair keeps the larger value — where a lane takes its partner's entry
//    only when that is STRICTLY on its side: equal values stay where they are.  That is not a stable sort: (1, .5, .5, .5, .2) comes out
//    as entries 4 1 3 2 0.  tests/test_mixfit.py holds this restatement against recorded np.argsort results for every tie pattern.
constexpr int mf_net_partner(int s, int i) { return s == 1 ? ((i & 4) | (3 - (i & 3))) : s == 3 ? 7 - i : s == 4 ? (i ^ 2) : (i ^ 1); }
constexpr bool mf_net_high(int s, int i) { return ((s == 3 ? 0xF0 : (s == 1 || s == 4) ? 0xCC : 0xAA) >> i) & 1; }

template <int N>
struct MfSimplex {
    double x[N + 1][4], f[N + 1];
    NS_HD void sort() {                                   // every index below is a constant after unrolling
        bool nan = false;
#pragma unroll
        for (int k = 0; k <= N; ++k) nan = nan || f[k] != f[k];
        if (nan) {
#pragma unroll
            for (int i = 1; i <= N; ++i)
#pragma unroll
                for (int j = i; j >= 1; --j)              // (a pair in order would end the textbook loop; going on changes nothing)
                    if (mf_less(f[j], f[j - 1])) {
                        const double t = f[j]; f[j] = f[j - 1]; f[j - 1] = t;
#pragma unroll
                        for (int c = 0; c < N; ++c) { const double u = x[j][c]; x[j][c] = x[j - 1][c]; x[j - 1][c] = u; }
                    }
            return;
        }
        double key[8]; uint32_t idx[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) { key[i] = i <= N ? f[i] : ns_bits_to_double(0x7ff0000000000000ull); idx[i] = (uint32_t)i; }
#pragma unroll
        for (int s = 0; s < 6; ++s) {
            double nk[8]; uint32_t ni[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int j = mf_net_partner(s, i);
                const bool take = mf_net_high(s, i) ? key[j] > key[i] : key[j] < key[i];
                nk[i] = take ? key[j] : key[i]; ni[i] = take ? idx[j] : idx[i];
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) { key[i] = nk[i]; idx[i] = ni[i]; }
        }
        double nx[N + 1][4];                              // (an entry equal to +inf ties with the padding and stays in the low lanes)
#pragma unroll
        for (int i = 0; i <= N; ++i)
#pragma unroll
            for (int c = 0; c < N; ++c) {
                double v = x[0][c];
#pragma unroll
                for (int k = 1; k <= N; ++k) v = idx[i] == (uint32_t)k ? x[k][c] : v;
                nx[i][c] = v;
            }
#pragma unroll
        for (int i = 0; i <= N; ++i) {
            f[i] = key[i];
#pragma unroll
            for (int c = 0; c < N; ++c) x[i][c] = nx[i][c];
        }
    }
};

// One search.  Obj: double operator()(const double (&)[4]) const and N.  out: x (entries beyond N are 0), fun, residual = the value at x,
// nfev, nit, status (0 converged, 1 maxfev, 2 maxiter).
template <class Obj>
NS_HD void mf_nelder_mead(const Obj &obj, const double *x0, uint32_t maxiter, uint32_t maxfev, ns_mixfit_fit &out) {
    constexpr int N = Obj::N;
    MfSimplex<N> s;
    uint32_t nfev = 0, nit = 1;
#pragma unroll
    for (int k = 0; k <= N; ++k) {
#pragma unroll
        for (int c = 0; c < 4; ++c) s.x[k][c] = c < N ? x0[c] : 0.0;
        if (k) s.x[k][k - 1] = s.x[k][k - 1] != 0.0 ? (1.0 + 0.05) * s.x[k][k - 1] : 0.00025;
        s.f[k] = ns_bits_to_double(0x7ff0000000000000ull);                       // np.inf until evaluated
    }
#pragma unroll
    for (int k = 0; k <= N; ++k) if (nfev < maxfev) { ++nfev; s.f[k] = obj(s.x[k]); }
    s.sort();
    while (nfev < maxfev && nit < maxiter) {
        bool small = true;
#pragma unroll
        for (int k = 1; k <= N; ++k) {
#pragma unroll
            for (int c = 0; c < N; ++c) small = small && mf_absdiff(s.x[k][c], s.x[0][c]) <= 1e-4;
            small = small && mf_absdiff(s.f[0], s.f[k]) <= 1e-4;
        }
        if (small) break;
        do {                                               // (one iteration; `break` = scipy's _MaxFuncCallError)
            double xbar[4] = {0.0, 0.0, 0.0, 0.0}, xt[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int c = 0; c < N; ++c) {
                double a = s.x[0][c];
#pragma unroll
                for (int k = 1; k < N; ++k) a = a + s.x[k][c];
                xbar[c] = a / (double)N;
            }
#pragma unroll
            for (int c = 0; c < N; ++c) xt[c] = 2.0 * xbar[c] - 1.0 * s.x[N][c];
            if (nfev >= maxfev) break;
            ++nfev;
            const double fxr = obj(xt);
            bool shrink = false;
            if (fxr < s.f[0]) {
                double xe[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int c = 0; c < N; ++c) xe[c] = 3.0 * xbar[c] - 2.0 * s.x[N][c];
                if (nfev >= maxfev) break;
                ++nfev;
                const double fxe = obj(xe);
                const bool e = fxe < fxr;
#pragma unroll
                for (int c = 0; c < N; ++c) s.x[N][c] = e ? xe[c] : xt[c];
                s.f[N] = e ? fxe : fxr;
            } else if (fxr < s.f[N - 1]) {
#pragma unroll
                for (int c = 0; c < N; ++c) s.x[N][c] = xt[c];
                s.f[N] = fxr;
            } else {
                const bool outside = fxr < s.f[N];
                double xc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int c = 0; c < N; ++c) xc[c] = outside ? 1.5 * xbar[c] - 0.5 * s.x[N][c] : 0.5 * xbar[c] + 0.5 * s.x[N][c];
                if (nfev >= maxfev) break;
                ++nfev;
                const double fxc = obj(xc);
                if (outside ? fxc <= fxr : fxc < s.f[N]) {
#pragma unroll
                    for (int c = 0; c < N; ++c) s.x[N][c] = xc[c];
                    s.f[N] = fxc;
                } else shrink = true;
            }
            bool refused = false;
            if (shrink) {
#pragma unroll
                for (int k = 1; k <= N; ++k) {
                    if (refused) continue;
#pragma unroll
                    for (int c = 0; c < N; ++c) s.x[k][c] = s.x[0][c] + 0.5 * (s.x[k][c] - s.x[0][c]);
                    if (nfev >= maxfev) { refused = true; continue; }
                    ++nfev;
                    s.f[k] = obj(s.x[k]);
                }
            }
            if (refused) break;
            ++nit;
        } while (false);
        s.sort();
    }
    double fun = s.f[0];
#pragma unroll
    for (int k = 1; k <= N; ++k) if (s.f[k] != s.f[k]) fun = mf_nan();
    if (fun != fun) fun = mf_nan();
#pragma unroll
    for (int c = 0; c < 4; ++c) out.x[c] = s.x[0][c];
    out.fun = fun; out.residual = s.f[0];
    out.nfev = nfev; out.nit = nit;
    out.status = nfev >= maxfev ? 1 : nit >= maxiter ? 2 : 0;
}

// evaluate-only: the objective at x0
template <class Obj>
NS_HD void mf_evaluate(const Obj &obj, const double *x0, ns_mixfit_fit &out) {
    double x[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) x[c] = c < Obj::N ? x0[c] : 0.0;
    const double f = obj(x);
#pragma unroll
    for (int c = 0; c < 4; ++c) out.x[c] = x[c];
    out.fun = f; out.residual = f; out.nfev = 1; out.nit = 0; out.status = 0;
}
