// Test shim (CPU tests only): the engine's quantification EM (nanosim_amd/csrc/ns_em.h — the code k_em_estep, k_em_accum and k_em_stop
// run per thread and per wavefront) compiled for the HOST behind the signature of ns_em_quantify, so that the iteration and the host
// module around the call are checked against the reference's fixture without a GPU.  A wavefront is one thread here; the slots are laid
// out as the host side of the call does.  Built by tests/test_quantify.py with g++ -ffp-contract=off into tests/_tmp/: as a shared
// library, and, with -DEM_MAIN, as a stand-alone program for -fsanitize=address,undefined that runs a problem it makes up itself.
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../include/nanosim_amd.h"
#include "../nanosim_amd/csrc/ns_em.h"

extern "C" int em_host_quantify(void *, const ns_em_problem *p, ns_em_result *out) {
    if (!p || !out) return -1;
    out->n_iter = 0; out->reserved = 0; out->n_nonfinite = 0; out->ms_kernel = 0;
    const uint32_t nt = p->n_targets, nm = p->n_multi;
    if (!nt || !(p->total > 0.0) || !(p->total * 100.0 < 9007199254740992.0) || !p->max_iter) return -1;
    if (!p->unique || !out->abundance || !out->count || !out->diff_trace || (nm && (!p->multi_off || !p->target || !p->weight))) return -1;
    uint64_t n_ent = 0;
    if (nm) {
        if (p->multi_off[0] != 0) return -1;
        for (uint32_t m = 0; m < nm; ++m) if (p->multi_off[m] >= p->multi_off[m + 1]) return -1;
        n_ent = p->multi_off[nm];
    }
    std::vector<uint64_t> tgt_off((size_t)nt + 1, 0), slot((size_t)n_ent);
    for (uint64_t e = 0; e < n_ent; ++e) { if (p->target[e] >= nt) return -1; ++tgt_off[p->target[e] + 1u]; }
    for (uint32_t t = 0; t < nt; ++t) tgt_off[t + 1] += tgt_off[t];
    {
        std::vector<uint64_t> next(tgt_off.begin(), tgt_off.end() - 1);
        for (uint64_t e = 0; e < n_ent; ++e) slot[e] = next[p->target[e]]++;
    }
    std::vector<double> a(nt, 100.0 / (double)nt), dabs(nt, 0.0), contrib((size_t)n_ent, 0.0);   // (exact sizes: a sanitizer sees a slot out of range)
    EmState S{0u, 0u, 0ull, 100.0 * (double)nt};
    for (uint32_t i = 0; i < p->max_iter; ++i) out->diff_trace[i] = 0.0;
    while (!S.stop) {
        for (uint32_t m = 0; m < nm; ++m) em_item_estep(a.data(), p->target, slot.data(), p->multi_off[m], p->multi_off[m + 1], p->weight[m], contrib.data());
        for (uint32_t t = 0; t < nt; ++t) {
            const double acc = em_fold(p->unique[t], contrib.data() + tgt_off[t], tgt_off[t + 1] - tgt_off[t]);
            em_target_step(acc, p->total, out->count + t, a.data() + t, dabs.data() + t);
        }
        double mn = a[0]; uint64_t bad = 0;
        for (uint32_t t = 0; t < nt; ++t) {
            mn = a[t] < mn ? a[t] : mn;
            if (!em_finite(a[t])) ++bad;
        }
        em_decide(&S, em_fold(0.0, dabs.data(), nt), mn, bad, p->factor, p->max_iter, out->diff_trace);
    }
    for (uint32_t t = 0; t < nt; ++t) out->abundance[t] = a[t];
    out->n_iter = S.n_iter; out->n_nonfinite = S.n_nonfinite;
    return 0;
}

// em_decide alone, for a table of hand-chosen states (tests/test_quantify.py: the exact ties of G:82 are hard to reach through a whole
// problem).  state: {diff, it} in, {diff, n_iter, stop} out; trace: max_iter doubles.
extern "C" void em_host_decide(double *diff, uint32_t *it, uint32_t *stop, double diff_tmp, double mn, uint64_t n_nonfinite, double factor,
                               uint32_t max_iter, double *trace) {
    EmState S{0u, *it, 0ull, *diff};
    em_decide(&S, diff_tmp, mn, n_nonfinite, factor, max_iter, trace);
    *diff = S.diff; *it = S.n_iter; *stop = S.stop;
}

#ifdef EM_MAIN
#include <stdio.h>
int main() {
    {   // em_host_decide at the last slot of an exact-size trace: iteration max_iter - 1 writes trace[max_iter - 1] and nothing behind it
        std::vector<double> tr(3, 0.0);
        double diff = 300.0; uint32_t it = 2, stop = 0;
        em_host_decide(&diff, &it, &stop, 1.5, 2.0, 0, 0.01, 3, tr.data());
        if (!(tr[2] == 1.5 && it == 3 && stop == 1 && diff == 1.5)) return 4;
    }
    // 130 targets, 700 items of 2 .. 6 candidates (duplicates among them) from a small generator; targets 5 and 77 stay without a read
    const uint32_t nt = 130, nm = 700;
    uint64_t x = 88172645463325252ull;
    auto next = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    std::vector<uint64_t> off{0}; std::vector<uint32_t> target; std::vector<double> weight, unique(nt, 0.0);
    double total = 0;
    for (uint32_t m = 0; m < nm; ++m) {
        const uint32_t k = 2u + (uint32_t)(next() % 5u);
        for (uint32_t j = 0; j < k; ++j) { uint32_t t = (uint32_t)(next() % nt); if (t == 5u || t == 77u) t = 6u; target.push_back(t); }
        off.push_back(target.size());
        const double w = 100.0 + (double)(next() % 900u);
        weight.push_back(w); total += w;
    }
    for (uint32_t t = 0; t < nt; ++t) if (t != 5u && t != 77u) { unique[t] = (double)(next() % 5000u); total += unique[t]; }
    for (int kind = 0; kind < 2; ++kind) {
        const uint32_t max_iter = kind ? 1000u : 100u;
        std::vector<double> ab(nt), cnt(nt), trace(max_iter);
        ns_em_problem P; memset(&P, 0, sizeof P);
        P.n_targets = nt; P.n_multi = nm; P.multi_off = off.data(); P.target = target.data(); P.weight = weight.data(); P.unique = unique.data();
        P.total = total; P.factor = kind ? 0.001 : 0.01; P.max_iter = max_iter; P.group = 10;
        ns_em_result R; memset(&R, 0, sizeof R);
        R.abundance = ab.data(); R.count = cnt.data(); R.diff_trace = trace.data();
        if (em_host_quantify(nullptr, &P, &R)) return 3;
        double sum = 0; for (double v : ab) sum += v;
        printf("%u %llu %.17g %.17g\n", R.n_iter, (unsigned long long)R.n_nonfinite, sum, trace[R.n_iter - 1]);
        P.n_multi = 0;
        if (em_host_quantify(nullptr, &P, &R)) return 3;
        printf("%u\n", R.n_iter);
    }
    return 0;
}
#endif
