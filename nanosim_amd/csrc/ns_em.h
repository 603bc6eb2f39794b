// ns_em.h — training side, abundance quantification ("Quantification: the EM in the reference's order"): EM_meta and EM_trans
// of src/get_primary_sam.py (G:44-142), one iteration as G:64-84 / G:108-127 write it.  G: = src/get_primary_sam.py of bcgsc/NanoSim v3.2.2.
//
// The problem: n_targets targets (species or transcripts) in the order of the reference's all_species dict, n_multi multi-mapping items in
// the order of its multi_mapping_list; item m has a weight (the aligned length for meta, 1.0 for trans: 1.0 * p == p, one code path) and
// the candidates target[multi_off[m] .. multi_off[m + 1]), duplicates kept.  unique[t] is an exact integer held as a double.
//
// The result of the reference depends on its summation order: its threshold is 0 as soon as one target has no read, so the loop ends
// where `diff` no longer shrinks — in rounding noise.  Every sum here is therefore the reference's, term by term, in its order:
//   E-step   (em_item_estep, one item per thread)  tot = ((0 + a[c0]) + a[c1]) + ...; p_j = a[c_j] / tot; contrib = weight * p_j, stored at
//            slot[e]: the slots of a target are contiguous and ordered by (item, position in its list), which is the order in which the
//            reference's `+=` reaches that target (G:71, G:114).
//   accumulate + M-step (em_fold, then em_target_step, one wavefront per target)  acc = unique[t]; acc = acc + contrib_k in slot order;
//            count[t] = acc; new = (acc * 100) / total  (G:74, G:117); dabs[t] = |new - a[t]|; a[t] = new (G:80 — nothing reads the old
//            value any more: the E-step of this iteration is over).
//   stop     (em_fold again, one wavefront)  diff_tmp = ((0 + dabs[0]) + dabs[1]) + ... in target order (G:75, G:118), then em_decide:
//            G:80-84 to the letter.
// em_fold leaves out terms that are 0.0: every sum here starts at a value >= +0.0 and has terms >= 0.0, and x + 0.0 == x for such x — the
// result is the same bit for bit, and the chain over the targets shrinks to the expressed ones.
// No fused multiply-add may be formed (the project builds with -ffp-contract=off; there is no a * b + c below anyway: products are stored
// before they are added), and the fp64 divide is the correctly rounded one.
// The code below compiles for the device (k_em_estep, k_em_accum, k_em_stop in ns_train.h) and, unchanged, for the host (tests/em_host.cpp),
// where a "wavefront" is one thread that owns all 64 lanes.
#pragma once
#include <math.h>
#include <stdint.h>
#include "ns_cs_hist.h"                                               // NS_CSH

#define NS_EM_CHUNK 64u                                                // W: the terms a wavefront loads at a time
#define NS_EM_DENSE 20u                                                // a chunk with more non-zero terms than this is folded lane by lane, zeros included

struct EmState {                                                       // lives on the device between the kernels of a call
    uint32_t stop, n_iter;
    uint64_t n_nonfinite;                                              // of new[] in the last executed iteration
    double diff;                                                       // G:62 / G:106: 100 * n_targets at first
};

// one item: the candidates target[lo .. hi); a[] the current abundances
NS_CSH void em_item_estep(const double *a, const uint32_t *target, const uint64_t *slot, uint64_t lo, uint64_t hi, double weight, double *contrib) {
    double tot = 0.0;
    for (uint64_t e = lo; e < hi; ++e) tot = tot + a[target[e]];
    for (uint64_t e = lo; e < hi; ++e) {
        const double p = a[target[e]] / tot;
        contrib[slot[e]] = weight * p;
    }
}

// acc + v[0] + v[1] + ... + v[n - 1], strictly left to right, terms equal to 0.0 left out (see above).  Device: called by all 64 lanes of a
// wavefront with the same arguments; lane j loads term 64 c + j of chunk c (coalesced), the chain runs through the chunk with cross-lane
// reads (v_readlane: the term comes through a scalar register), and every lane returns the same value.
NS_CSH double em_fold(double acc, const double *v, uint64_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t lane = threadIdx.x & 63u;
    double x = lane < n ? v[lane] : 0.0;
    for (uint64_t k = 0; k < n; k += NS_EM_CHUNK) {
        const uint64_t kn = k + NS_EM_CHUNK + lane;
        const double xn = kn < n ? v[kn] : 0.0;                       // the next chunk is in flight while the chain runs through this one
        const unsigned long long xb = (unsigned long long)__double_as_longlong(x);
        uint64_t live = __ballot(x != 0.0);                            // (a NaN is a term: it has to show in the result)
        if (__builtin_popcountll(live) > (int)NS_EM_DENSE) {
            // most terms count: all 64 lanes with constant lane numbers (x + 0.0 == x: the zeros change nothing); the cross-lane reads
            // do not depend on the chain and run ahead of it, so a term costs one dependent add
#pragma unroll
            for (int j = 0; j < (int)NS_EM_CHUNK; ++j) {
                const unsigned long long lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)xb, j);
                const unsigned long long hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(xb >> 32), j);
                acc = acc + __longlong_as_double((long long)(hi << 32 | lo));
            }
        } else {
            while (live) {                                             // (the mask and the lane index are the wavefront's: scalar registers)
                const int j = __builtin_ctzll(live);
                const unsigned long long lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)xb, j);
                const unsigned long long hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(xb >> 32), j);
                acc = acc + __longlong_as_double((long long)(hi << 32 | lo));
                live &= live - 1u;
            }
        }
        x = xn;
    }
#else
    for (uint64_t k = 0; k < n; ++k) if (v[k] != 0.0) acc = acc + v[k];
#endif
    return acc;
}

// what one target takes from its sum (G:74-75, 80 / G:117-118, 123)
NS_CSH void em_target_step(double acc, double total, double *count, double *a, double *dabs) {
    const double v = (acc * 100.0) / total;
    *count = acc;
    *dabs = fabs(v - *a);
    *a = v;
}

// G:80-84 / G:123-127 behind `abundance_list = abundance_list_tmp`: the trace entry of this iteration, the decision, the iteration count.
// mn = min(new); a NaN among new[] ends the loop too (every comparison with it is false: the reference would run to its last iteration
// and write `nan`; the caller raises instead).
NS_CSH void em_decide(EmState *S, double diff_tmp, double mn, uint64_t n_nonfinite, double factor, uint32_t max_iter, double *diff_trace) {
    const uint32_t it = S->n_iter;
    if (it < max_iter) diff_trace[it] = diff_tmp;
    const double thres = mn * factor;
    S->n_nonfinite = n_nonfinite;
    if (diff_tmp <= thres || S->diff - diff_tmp < thres || n_nonfinite) S->stop = 1u;
    else S->diff = diff_tmp;
    S->n_iter = it + 1u;
    if (it + 1u >= max_iter) S->stop = 1u;
}

NS_CSH bool em_finite(double x) { return x - x == 0.0; }
