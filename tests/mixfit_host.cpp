// Test shim (CPU tests only): the engine's mixture fit (nanosim_amd/csrc/ns_mixfit.h — the code a wavefront of k_mixfit runs per start)
// compiled for the HOST behind the signature of ns_mixture_fit, so that the objectives, the search and the host module around the call are
// checked against the reference's fixture and against scipy without a GPU: one thread walks the 64 lanes of a tile as a 64-entry array, in
// the order the header fixes.  Built by tests/test_mixfit.py (the compiler's host pass only, -ffp-contract=off) into tests/_tmp/.
// mixfit_host_hand puts hand-made functions behind the same simplex code.  With -DMIXFIT_MAIN the file is a stand-alone program for
// the sanitizer run: it reads `kind n_bins n_starts`, the CDF and the starts from standard input into heap buffers of exactly that size.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <thread>
#include <vector>
#include "../include/nanosim_amd.h"
#include "../nanosim_amd/csrc/ns_mixfit.h"

extern "C" int mixfit_host_fit(void *, int kind, const double *cdf, uint32_t n_bins, const double *starts, uint32_t n_starts, int mode,
                               ns_mixfit_result *out) {
    if (!out || !out->fits || !cdf || !starts) return -1;
    if ((kind != NS_MIXFIT_MISMATCH && kind != NS_MIXFIT_INDEL) || (mode != NS_MIXFIT_FIT && mode != NS_MIXFIT_EVALUATE)) return -1;
    if (!n_bins || n_bins > MF_MAX_BINS || !n_starts) return -1;
    out->ms_kernel = 0;
    std::vector<double> lnf(n_bins);
    mf_lnfact_table(lnf.data(), n_bins);
    auto run = [&](uint32_t first, uint32_t step) {                  // the starts are independent: a few threads share them
        for (uint32_t s = first; s < n_starts; s += step) {
            ns_mixfit_fit r;
            r.reserved = 0;
            if (kind == NS_MIXFIT_MISMATCH) {
                const MfMis obj{cdf, lnf.data(), n_bins};
                if (mode == NS_MIXFIT_EVALUATE) mf_evaluate(obj, starts + (size_t)s * 3, r); else mf_nelder_mead(obj, starts + (size_t)s * 3, 600u, 600u, r);
            } else {
                const MfIndel obj{cdf, lnf.data(), n_bins};
                if (mode == NS_MIXFIT_EVALUATE) mf_evaluate(obj, starts + (size_t)s * 4, r); else mf_nelder_mead(obj, starts + (size_t)s * 4, 800u, 800u, r);
            }
            out->fits[s] = r;
        }
    };
    const uint32_t hw = std::thread::hardware_concurrency();
    const uint32_t n_thr = mode == NS_MIXFIT_EVALUATE || n_starts < 64u ? 1u : (hw < 2u ? 1u : hw > 8u ? 8u : hw);
    std::vector<std::thread> pool;
    for (uint32_t t = 1; t < n_thr; ++t) pool.emplace_back(run, t, n_thr);
    run(0, n_thr);
    for (std::thread &t : pool) t.join();
    return 0;
}

// ---- hand cases on the search skeleton: tests/test_mixfit.py restates the functions operation by operation ----
static const double HAND_A[4] = {0.3, -1.25, 2.0, 0.75}, HAND_B[4] = {1.0, 3.5, 0.5, 10.0};
template <int D> struct HandQuadratic {                       // sum of b (x - a)^2, accumulated left to right
    static constexpr int N = D;
    double operator()(const double (&x)[4]) const {
        double acc = 0.0;
        for (int c = 0; c < D; ++c) { const double d = x[c] - HAND_A[c]; acc = acc + (HAND_B[c] * d) * d; }
        return acc;
    }
};
template <int D> struct HandBox {                             // the same, NaN outside the box |x - a| <= 1.5 in every coordinate
    static constexpr int N = D;
    double operator()(const double (&x)[4]) const {
        for (int c = 0; c < D; ++c) { const double d = x[c] - HAND_A[c]; if (d > 1.5 || d < -1.5) return mf_nan(); }
        return HandQuadratic<D>()(x);
    }
};
template <int D> struct HandSteps {                           // the same in steps of 1/4, rounded down: vertices, reflections and contractions TIE
    static constexpr int N = D;
    double operator()(const double (&x)[4]) const { return floor(HandQuadratic<D>()(x) * 4.0) / 4.0; }
};
struct HandSlope {                                             // steep below x[0] = -2e-5, gentle above it, the other two coordinates break ties:
    static constexpr int N = 3;                               // the simplex GROWS down the slope until its size meets the 1e-4 of the x test
    double operator()(const double (&x)[4]) const {
        const double a = x[0], t = -2e-5;
        const double g = a < t ? -1000.0 * a : -1000.0 * t - 0.5 * (a - t);
        return (g - 0.01 * x[1]) - 0.001 * x[2];
    }
};
struct HandCliff {                                             // `height` where x[0] > 1.02e-3, else 0: the first simplex's values differ by exactly `height`
    static constexpr int N = 3;
    double height;
    double operator()(const double (&x)[4]) const { return x[0] > 1.02e-3 ? height : 0.0; }
};
extern "C" int mixfit_host_hand(int which, int dim, const double *x0, uint32_t maxiter, uint32_t maxfev, ns_mixfit_fit *out) {
    out->reserved = 0;
    if (which == 0 && dim == 3) mf_nelder_mead(HandQuadratic<3>(), x0, maxiter, maxfev, *out);
    else if (which == 0 && dim == 4) mf_nelder_mead(HandQuadratic<4>(), x0, maxiter, maxfev, *out);
    else if (which == 1 && dim == 3) mf_nelder_mead(HandBox<3>(), x0, maxiter, maxfev, *out);
    else if (which == 1 && dim == 4) mf_nelder_mead(HandBox<4>(), x0, maxiter, maxfev, *out);
    else if (which == 2 && dim == 3) mf_nelder_mead(HandSteps<3>(), x0, maxiter, maxfev, *out);
    else if (which == 2 && dim == 4) mf_nelder_mead(HandSteps<4>(), x0, maxiter, maxfev, *out);
    else if (which == 3 && dim == 3) mf_nelder_mead(HandSlope(), x0, maxiter, maxfev, *out);
    else if (which == 4 && dim == 3) mf_nelder_mead(HandCliff{1e-4}, x0, maxiter, maxfev, *out);
    else if (which == 5 && dim == 3) mf_nelder_mead(HandCliff{1.0000000000000002e-4}, x0, maxiter, maxfev, *out);
    else return -1;
    return 0;
}

// the order MfSimplex::sort gives n = 4 or 5 values: order[i] = the entry that ends in place i
extern "C" int mixfit_host_argsort(int n, const double *f, uint32_t *order) {
    auto run = [&](auto &s) {
        for (int k = 0; k < n; ++k) { s.f[k] = f[k]; for (int c = 0; c < 4; ++c) s.x[k][c] = (double)k; }
        s.sort();
        for (int k = 0; k < n; ++k) order[k] = (uint32_t)s.x[k][0];
    };
    if (n == 4) { MfSimplex<3> s; run(s); } else if (n == 5) { MfSimplex<4> s; run(s); } else return -1;
    return 0;
}

#ifdef MIXFIT_MAIN
int main() {
    int kind; unsigned n_bins, n_starts;
    if (scanf("%d %u %u", &kind, &n_bins, &n_starts) != 3) return 2;
    const unsigned dim = kind == NS_MIXFIT_MISMATCH ? 3u : 4u;
    double *cdf = (double *)malloc(sizeof(double) * n_bins), *starts = (double *)malloc(sizeof(double) * n_starts * dim);
    ns_mixfit_fit *fits = (ns_mixfit_fit *)malloc(sizeof(ns_mixfit_fit) * n_starts);
    if (!cdf || !starts || !fits) return 2;
    for (unsigned i = 0; i < n_bins; ++i) if (scanf("%lf", &cdf[i]) != 1) return 2;
    for (unsigned i = 0; i < n_starts * dim; ++i) if (scanf("%lf", &starts[i]) != 1) return 2;
    ns_mixfit_result out{fits, 0.0};
    int rc = mixfit_host_fit(nullptr, kind, cdf, n_bins, starts, n_starts, NS_MIXFIT_EVALUATE, &out);
    double sum = 0.0;
    for (unsigned i = 0; i < n_starts; ++i) if (fits[i].fun == fits[i].fun) sum += fits[i].fun;
    if (!rc) rc = mixfit_host_fit(nullptr, kind, cdf, n_bins, starts, n_starts, NS_MIXFIT_FIT, &out);
    unsigned long evals = 0;
    for (unsigned i = 0; i < n_starts; ++i) evals += fits[i].nfev;
    printf("rc %d objective sum %.17g evaluations %lu\n", rc, sum, evals);
    free(fits); free(starts); free(cdf);
    return rc ? 1 : 0;
}
#endif
