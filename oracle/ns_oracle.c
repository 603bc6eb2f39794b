/*
 * ns_oracle.c — CPU restatement of NanoSim's per-read generation path.
 *
 * >>> TEST INFRASTRUCTURE ONLY. <<<  Nothing in nanosim_amd/ (the product) links, imports or calls
 * this file.  Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may use it, and
 * only as the checker.
 *
 * Every function cites the reference lines it follows (S: = /root/reference/src/simulator.py,
 * mm: = src/mixed_model.py, hp: = src/model_homopolymer_lengths.py, bq: = src/model_base_qualities.py,
 * B: = src/besthit_to_histogram.py — the training side's counting loop, at the end of the file).
 *
 * Two draw sources:
 *   NSO_PHILOX  counter-based draws with the layout of DESIGN.md §4 — the HIP kernels must reproduce
 *               these results bit-for-bit;
 *   NSO_TAPE    uniforms / run lengths / normals are popped from tapes recorded while running the REAL
 *               reference (tests/golden/make_golden.py) — this is how the restatement is pinned.
 *
 * Parity status: pinned against outputs of the imported reference (the .json fixtures under tests/golden/, reference_hist.json.gz);
 * the reference itself has no tests.
 *
 * Build: make -C oracle   (gcc -O2 -ffp-contract=off; fma() only where written).
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/nanosim_amd.h"

/* ------------------------------------------------------------------------------------------------
 * Philox4x32-10 (Salmon et al. 2011) and the counter layout
 * ---------------------------------------------------------------------------------------------- */
enum {
    ST_NSEG = 1, ST_REFLEN = 2, ST_GAPLEN = 3, ST_HT = 4, ST_RATIO = 5, ST_STRAND = 6, ST_EVENT = 7,
    ST_UEVENT = 8, ST_POS = 9, ST_IUPAC = 10, ST_SUB = 11, ST_INS = 12, ST_QUAL = 13, ST_HTQ = 14,
    ST_HEAD = 15, ST_TAIL = 16, ST_HPLEN = 17, ST_HPMIS = 18, ST_HPQ = 19, ST_ULEN = 20
};
#define NSO_GAP_SEG 128u          /* gaps use seg ids 128+g */
#define NSO_MAX_ATTEMPT 1000u
#define NSO_EPOCH_FAILS 64u
#define NSO_KDE_RETRY 64u
#define NSO_POS_RETRY 64u

void nso_philox(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t out[4]) {
    for (int r = 0; r < 10; ++r) {
        uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        uint32_t n1 = (uint32_t)p1;
        uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        uint32_t n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

typedef struct nso_draw {
    int mode;                 /* 0 = Philox, 1 = tape */
    uint64_t seed, read;
    const double *tape_u; uint64_t n_u, i_u;      /* uniforms in consumption order */
    const int64_t *tape_n; uint64_t n_n, i_n;     /* run lengths returned by pois_geom / wei_geom */
    const double *tape_z; uint64_t n_z, i_z;      /* normal variates */
    int tape_err;
} nso_draw;

static void philox_at(const nso_draw *d, uint32_t stream, uint32_t seg, uint32_t attempt, uint32_t idx,
                      uint32_t sub, uint32_t w[4]) {
    uint32_t c3 = (uint32_t)((d->read >> 32) & 0xffu) << 24 | (stream & 0x3fu) << 18 | (seg & 0xffu) << 10 |
                  (attempt & 0x3ffu);
    nso_philox((uint32_t)d->seed, (uint32_t)(d->seed >> 32), idx, sub, (uint32_t)d->read, c3, w);
}
static inline double u32_to_p(uint32_t x) { return ((double)x + 0.5) * 0x1p-32; }
static inline double u53_to_p(uint32_t a, uint32_t b) {
    return ((double)(((uint64_t)(a >> 5) << 26) | (uint64_t)(b >> 6)) + 0.5) * 0x1p-53;
}
static double tape_u(nso_draw *d) {
    if (d->i_u >= d->n_u) { d->tape_err = 1; return 0.5; }
    return d->tape_u[d->i_u++];
}
static int64_t tape_n(nso_draw *d) {
    if (d->i_n >= d->n_n) { d->tape_err = 1; return 1; }
    return d->tape_n[d->i_n++];
}
static double tape_z(nso_draw *d) {
    if (d->i_z >= d->n_z) { d->tape_err = 1; return 0.0; }
    return d->tape_z[d->i_z++];
}

/* ------------------------------------------------------------------------------------------------
 * exact-operation math (only + - * / sqrt fma and bit moves, so CPU and GPU agree bit-for-bit)
 * ---------------------------------------------------------------------------------------------- */
double nso_log(double x) {
    uint64_t b; memcpy(&b, &x, 8);
    int e = (int)((b >> 52) & 0x7ff) - 1023;
    b = (b & 0x000fffffffffffffull) | 0x3ff0000000000000ull;
    double m; memcpy(&m, &b, 8);
    if (m > 1.4142135623730951) { m *= 0.5; e += 1; }
    double s = (m - 1.0) / (m + 1.0);
    double z = s * s;
    double r = 1.0 / 23.0;
    r = fma(r, z, 1.0 / 21.0); r = fma(r, z, 1.0 / 19.0); r = fma(r, z, 1.0 / 17.0);
    r = fma(r, z, 1.0 / 15.0); r = fma(r, z, 1.0 / 13.0); r = fma(r, z, 1.0 / 11.0);
    r = fma(r, z, 1.0 / 9.0);  r = fma(r, z, 1.0 / 7.0);  r = fma(r, z, 1.0 / 5.0);
    r = fma(r, z, 1.0 / 3.0);  r = fma(r, z, 1.0);
    return fma((double)e, 0.6931471805599453, 2.0 * s * r);
}

double nso_exp(double y) {
    if (y > 700.0) y = 700.0;
    if (y < -700.0) y = -700.0;
    double k = floor(fma(y, 1.4426950408889634, 0.5));
    double r = fma(-k, 6.93147180369123816490e-01, y);
    r = fma(-k, 1.90821492927058770002e-10, r);
    double p = 1.0 / 6227020800.0;                 /* 1/13! */
    p = fma(p, r, 1.0 / 479001600.0); p = fma(p, r, 1.0 / 39916800.0); p = fma(p, r, 1.0 / 3628800.0);
    p = fma(p, r, 1.0 / 362880.0);    p = fma(p, r, 1.0 / 40320.0);    p = fma(p, r, 1.0 / 5040.0);
    p = fma(p, r, 1.0 / 720.0);       p = fma(p, r, 1.0 / 120.0);      p = fma(p, r, 1.0 / 24.0);
    p = fma(p, r, 1.0 / 6.0);         p = fma(p, r, 0.5);              p = fma(p, r, 1.0);
    p = fma(p, r, 1.0);
    uint64_t b = (uint64_t)((int64_t)k + 1023) << 52;
    double sc; memcpy(&sc, &b, 8);
    return p * sc;
}

/* inverse normal CDF, P. J. Acklam's rational approximation (rel. err 1.15e-9) */
double nso_norminv(double p) {
    static const double a[6] = {-3.969683028665376e+01, 2.209460984245205e+02, -2.759285104469687e+02,
                                1.383577518672690e+02, -3.066479806614716e+01, 2.506628277459239e+00};
    static const double b[5] = {-5.447609879822406e+01, 1.615858368580409e+02, -1.556989798598866e+02,
                                6.680131188771972e+01, -1.328068155288572e+01};
    static const double c[6] = {-7.784894002430293e-03, -3.223964580411365e-01, -2.400758277161838e+00,
                                -2.549732539343734e+00, 4.374664141464968e+00, 2.938163982698783e+00};
    static const double dd[4] = {7.784695709041462e-03, 3.224671290700398e-01, 2.445134137142996e+00,
                                 3.754408661907416e+00};
    const double plow = 0.02425;
    if (p < plow || p > 1.0 - plow) {
        double t = (p < plow) ? p : 1.0 - p;
        double q = sqrt(-2.0 * nso_log(t));
        double num = c[0];
        for (int i = 1; i < 6; ++i) num = fma(num, q, c[i]);
        double den = dd[0];
        for (int i = 1; i < 4; ++i) den = fma(den, q, dd[i]);
        den = fma(den, q, 1.0);
        double x = num / den;
        return (p < plow) ? x : -x;
    }
    double q = p - 0.5, r = q * q;
    double num = a[0];
    for (int i = 1; i < 6; ++i) num = fma(num, r, a[i]);
    double den = b[0];
    for (int i = 1; i < 5; ++i) den = fma(den, r, b[i]);
    den = fma(den, r, 1.0);
    return num * q / den;
}

/* float -> int64 with a result for every input (ns_rng.h ns_f64_to_i64_sat): C's truncation where that is defined, saturated above
 * and below the int64 range, 0 for NaN.  A plain (int64_t)x out of range is undefined, and x86 and gfx950 resolve it differently. */
int64_t nso_f64_to_i64_sat(double x) {
    if (!(x == x)) return 0;
    if (x >= 9223372036854775808.0) return INT64_MAX;
    if (x < -9223372036854775808.0) return INT64_MIN;
    return (int64_t)x;
}
/* a drawn length above NSO_LEN_DRAW_MAX is no valid draw: -1 (ns_len_draw) */
#define NSO_LEN_DRAW_MAX 0x3fffffffll
static int64_t len_draw(double x) {
    const int64_t v = nso_f64_to_i64_sat(x);
    return v > NSO_LEN_DRAW_MAX ? -1 : v;
}
/* edge counters for the tests (tests/test_gpu_extremes.py proves its cases reach their edge): not thread-safe, reset by the caller */
enum { NSO_EDGE_ULEN_LONG = 0,    /* unaligned length draws above max_len or 0x3fffffff (no valid draw) */
       NSO_EDGE_ULEN_HUGE = 1,    /* ... of 2^31 or more (where a plain cast differs between x86 and gfx950) */
       NSO_EDGE_REM_SAT = 2,      /* head/tail remainders saturated at 0x3fffffff */
       NSO_EDGE_REM_HUGE = 3,     /* ... drawn at 2^31 or more */
       NSO_EDGE_LEN_HUGE = 4,     /* aligned / --perfect length draws of 2^31 or more (rejected by the max_len filter) */
       NSO_EDGE_N = 8 };
static uint64_t nso_edges[NSO_EDGE_N];
void nso_edge_counts(uint64_t *out, int reset) {
    for (int i = 0; i < NSO_EDGE_N; ++i) { if (out) out[i] = nso_edges[i]; if (reset) nso_edges[i] = 0; }
}

/* ------------------------------------------------------------------------------------------------
 * table look-ups
 * ---------------------------------------------------------------------------------------------- */
/* ECDF look-up of S:1845-1849 / S:1895-1898: segment with lo < p <= hi;
 * value = floor((p-lo)/(hi-lo)*(vhi-vlo)+vlo).  p above the last edge is clamped onto it (the
 * reference would reuse a stale value or raise; DESIGN.md "conscious fixes"). */
int64_t nso_ecdf_lookup(const double *hi, const double *vhi, uint32_t n, double vlo0, double p) {
    uint32_t lo_i = 0, hi_i = n;            /* first s with p <= hi[s] */
    while (lo_i < hi_i) {
        uint32_t mid = (lo_i + hi_i) >> 1;
        if (p <= hi[mid]) hi_i = mid; else lo_i = mid + 1;
    }
    uint32_t s = lo_i;
    if (s >= n) { s = n - 1; p = hi[s]; }
    double plo = s ? hi[s - 1] : 0.0;
    double vlo = s ? vhi[s - 1] : vlo0;
    return (int64_t)floor((p - plo) / (hi[s] - plo) * (vhi[s] - vlo) + vlo);
}

/* inverse-CDF table: value = 1 + #{j : p > cdf[j]}, capped at n */
static int64_t table_value(const double *cdf, uint32_t n, double p) {
    uint32_t lo = 0, hi = n;                /* first j with p <= cdf[j] */
    while (lo < hi) {
        uint32_t mid = (lo + hi) >> 1;
        if (p <= cdf[mid]) hi = mid; else lo = mid + 1;
    }
    if (lo >= n) lo = n - 1;
    return (int64_t)lo + 1;
}

/* transition pick, S:1860-1864: first of mis [0,a), ins [a,a+b), del [1-c,1) with lo <= p < hi.
 * If no interval matches (rounding gap) the reference keeps a stale variable; we fall to del when
 * p >= a+b, else ins. */
static int trans_pick(const double row[3], double p) {
    if (0.0 <= p && p < row[0]) return NS_MIS;
    if (row[0] <= p && p < row[1]) return NS_INS;
    if (row[2] <= p && p < 1.0) return NS_DEL;
    return (p >= row[1]) ? NS_DEL : NS_INS;
}

/* mm:41-49 pois_geom / mm:52-63 wei_geom through the inverse-CDF tables */
static int64_t run_length(const ns_model_tables *t, int type, double p_mix, double p_len) {
    int comp = (p_mix < t->mix_w[type]) ? 0 : 1;          /* tmp_rand < weight */
    return table_value(t->mix_cdf[type][comp], t->mix_n[type][comp], p_len);
}

/* ------------------------------------------------------------------------------------------------
 * error_list (S:1833-1916)
 * ---------------------------------------------------------------------------------------------- */
typedef struct nso_elist {
    int64_t l_new, middle_ref;
    int64_t e_count[3];       /* match, mis, ins (fastq only) */
    uint64_t n_ev;
    int64_t shift;            /* sum(ins - del) over the stored events */
    int overflow;
    int range;                /* an event outside the fields of ns_event (NS_EV_LEN_MAX, the 18-bit shift): the attempt is dropped */
} nso_elist;

static void push_event(ns_event *ev, uint64_t cap, nso_elist *r, int64_t pos, int type, int64_t len) {
    if (len > (int64_t)NS_EV_LEN_MAX || r->shift < -(int64_t)NS_EV_SHIFT_BIAS || r->shift >= (int64_t)NS_EV_SHIFT_BIAS) r->range = 1;
    if (len > (int64_t)NS_EV_LEN_MAX) len = NS_EV_LEN_MAX;
    if (ev && r->n_ev < cap) {
        ev[r->n_ev].pos = (uint32_t)pos;
        ev[r->n_ev].info = NS_EV_PACK(len, type, r->shift);
    } else if (ev) r->overflow = 1;
    if (type == NS_INS) r->shift += len; else if (type == NS_DEL) r->shift -= len;
    r->n_ev++;
}

void nso_error_list(const ns_model_tables *t, int64_t m_ref, int fastq, nso_draw *d, uint32_t seg,
                    uint32_t attempt, ns_event *ev, uint64_t cap, nso_elist *r) {
    uint32_t w[4];
    memset(r, 0, sizeof *r);
    int64_t l_new = m_ref, pos = 0, middle_ref = m_ref;
    int state = NS_ST_START;
    /* first match from m_ht_list, floored at 2 (S:1843-1850) */
    double p;
    if (d->mode) p = tape_u(d); else { philox_at(d, ST_EVENT, seg, attempt, 0, 0, w); p = u32_to_p(w[0]); }
    int64_t prev_match = nso_ecdf_lookup(t->fm_hi, t->fm_vhi, t->fm_nseg, t->fm_vlo0, p);
    if (prev_match < 2) prev_match = 2;
    pos += prev_match;
    if (fastq) r->e_count[0] += (prev_match > middle_ref) ? middle_ref : prev_match;     /* S:1852-1856 */
    uint32_t it = 1;
    int64_t last_ins_pos = -1;          /* collision of two insertions on key pos-0.5 (S:1882) */
    while (pos < middle_ref) {                                                             /* S:1858 */
        double p_err, p_mix = 0, p_len = 0, p_match = 0;
        if (!d->mode) {
            philox_at(d, ST_EVENT, seg, attempt, it, 0, w);
            p_err = u32_to_p(w[0]); p_mix = u32_to_p(w[1]); p_len = u32_to_p(w[2]); p_match = u32_to_p(w[3]);
        } else p_err = tape_u(d);
        int error = trans_pick(t->trans[state], p_err);                                    /* S:1860-1864 */
        int64_t step = d->mode ? tape_n(d) : run_length(t, error, p_mix, p_len);           /* S:1866-1873 */
        if (error == NS_INS) l_new += step; else if (error == NS_DEL) l_new -= step;
        if (error != NS_INS) {                                                             /* S:1875-1880 */
            push_event(ev, cap, r, pos, error, step);
            pos += step;
            if (pos >= middle_ref) { l_new += pos - middle_ref; middle_ref = pos; }
        } else {                                                                           /* S:1881-1882 */
            if (last_ins_pos == pos && r->n_ev > 0) {         /* same dict key: the later entry replaces */
                r->n_ev--;
                if (ev && r->n_ev < cap) r->shift -= NS_EV_LEN(ev[r->n_ev].info); else r->overflow = 1;
            }
            push_event(ev, cap, r, pos, NS_INS, step);
            last_ins_pos = pos;
        }
        state = NS_ST_MIS + error;                                                         /* S:1884 */
        if (fastq) {                                                                       /* S:1886-1888 */
            if (error == NS_MIS) r->e_count[1] += step; else if (error == NS_INS) r->e_count[2] += step;
        }
        /* next match length from the bin of prev_match; falls through to the last bin (S:1891-1893) */
        uint32_t b = 0;
        for (; b < t->mm_nbins; ++b)
            if (t->mm_bin_lo[b] <= prev_match && prev_match < t->mm_bin_hi[b]) break;
        if (b >= t->mm_nbins) b = t->mm_nbins - 1;
        if (d->mode) p_match = tape_u(d);
        uint32_t o = t->mm_seg_off[b];
        step = nso_ecdf_lookup(t->mm_hi + o, t->mm_vhi + o, t->mm_seg_off[b + 1] - o, t->mm_vlo0[b], p_match);
        if (prev_match == 0 && step == 0) step = 1;                                        /* S:1900-1901 */
        prev_match = step;
        if (fastq) r->e_count[0] += step;
        if (pos + prev_match > middle_ref) { l_new += pos + prev_match - middle_ref; middle_ref = pos + prev_match; }
        pos += prev_match;
        if (prev_match == 0) state += 3;                                                   /* S:1913-1914 */
        else last_ins_pos = -1;
        ++it;
    }
    r->l_new = l_new; r->middle_ref = middle_ref;
}

/* ------------------------------------------------------------------------------------------------
 * unaligned_error_list (S:1784-1830) with the event rewrite of DESIGN.md §5.3: an insertion at key
 * pos+0.1 followed by mis/del at key pos is applied by mutate_read to the ALREADY INSERTED bases
 * (descending key order, S:1960); the equivalent non-overlapping events are emitted here.
 * ---------------------------------------------------------------------------------------------- */
void nso_unaligned_error_list(const ns_model_tables *t, int64_t m_ref, nso_draw *d, uint32_t seg,
                              uint32_t attempt, ns_event *ev, uint64_t cap, nso_elist *r) {
    uint32_t w[4];
    memset(r, 0, sizeof *r);
    int64_t l_new = m_ref, pos = 0, middle_ref = m_ref;
    int64_t pend_ins = 0;                 /* merged insertion waiting at pos (last_is_ins) */
    r->l_new = l_new; r->middle_ref = middle_ref;
    if (m_ref <= 0) return;               /* S:1793-1794 (negative lengths never enter the loop either) */
    uint32_t it = 0;
    while (pos < middle_ref) {
        double p, p_mix = 0, p_len = 0;
        if (!d->mode) {
            philox_at(d, ST_UEVENT, seg, attempt, it, 0, w);
            p = u32_to_p(w[0]); p_mix = u32_to_p(w[1]); p_len = u32_to_p(w[2]);
        } else p = tape_u(d);
        ++it;
        /* error_rate = {(0,0.4): match, (0.4,0.7): mis, (0.7,0.85): ins, (0.85,1): del}, lo <= p < hi */
        int type = (p < 0.4) ? 3 : (p < 0.7) ? NS_MIS : (p < 0.85) ? NS_INS : NS_DEL;
        int64_t step = 1;
        if (type != 3) step = d->mode ? tape_n(d) : run_length(t, type, p_mix, p_len);
        if (type == NS_INS) { pend_ins += step; l_new += step; continue; }   /* S:1808-1815 */
        if (type == NS_DEL) l_new -= step;
        int64_t L = pend_ins; pend_ins = 0;
        if (type == 3) {
            if (L) push_event(ev, cap, r, pos + 1, NS_INS, L);
        } else if (type == NS_MIS) {
            if (!L) push_event(ev, cap, r, pos, NS_MIS, step);
            else {
                push_event(ev, cap, r, pos, NS_MIS, 1);
                push_event(ev, cap, r, pos + 1, NS_INS, L);
                if (step - 1 > L) push_event(ev, cap, r, pos + 1, NS_MIS, step - 1 - L);
            }
        } else {
            if (!L) push_event(ev, cap, r, pos, NS_DEL, step);
            else {
                int64_t dl = step - L; if (dl < 1) dl = 1;
                push_event(ev, cap, r, pos, NS_DEL, dl);
                if (L - (step - 1) > 0) push_event(ev, cap, r, pos + 1, NS_INS, L - (step - 1));
            }
        }
        pos += step;
        if (pos > middle_ref) { l_new += pos - middle_ref; middle_ref = pos; }               /* S:1826-1828 */
    }
    r->l_new = l_new; r->middle_ref = middle_ref;
}

/* ------------------------------------------------------------------------------------------------
 * letters
 * ---------------------------------------------------------------------------------------------- */
static const char BASES[4] = {'A', 'T', 'C', 'G'};        /* S:49 */
static int base_rank(uint8_t c) { return c == 'A' ? 0 : c == 'T' ? 1 : c == 'C' ? 2 : c == 'G' ? 3 : -1; }

/* case_convert (S:743-755): members in the reference's list order */
static int iupac_members(uint8_t c, char out[4]) {
    const char *m;
    switch (c) {
        case 'Y': m = "CT"; break; case 'R': m = "AG"; break; case 'W': m = "AT"; break;
        case 'S': m = "GC"; break; case 'K': m = "TG"; break; case 'M': m = "CA"; break;
        case 'D': m = "AGT"; break; case 'V': m = "ACG"; break; case 'H': m = "ACT"; break;
        case 'B': m = "CGT"; break; case 'N': m = "ATCG"; break; case 'X': m = "ATCG"; break;
        default: return 0;
    }
    int n = (int)strlen(m);
    memcpy(out, m, (size_t)n);
    return n;
}
/* normalisation the engine applies once at load time: upper-case; anything that is neither ACGT nor an
 * IUPAC code becomes N */
uint8_t nso_normalise_base(uint8_t c) {
    if (c >= 'a' && c <= 'z') c = (uint8_t)(c - 32);
    char tmp[4];
    if (base_rank(c) >= 0 || iupac_members(c, tmp)) return c;
    return 'N';
}
static uint8_t resolve_base(uint8_t c, nso_draw *d, uint32_t seg, uint32_t attempt, uint64_t x) {
    char mem[4];
    int n = iupac_members(c, mem);
    if (!n) return c;
    uint32_t j;
    if (d->mode) j = (uint32_t)(tape_u(d) * n);
    else { uint32_t w[4]; philox_at(d, ST_IUPAC, seg, attempt, (uint32_t)(x >> 2), 0, w); j = (uint32_t)(((uint64_t)w[x & 3] * (uint32_t)n) >> 32); }
    return (uint8_t)mem[j];
}
/* Payload letters of event j of a piece: one 32-bit word per event —
 *   word(j, 0) = Philox(ST_SUB, seg, attempt, idx = j>>2).w[j&3]   (letters 0..15)
 *   word(j, c) = Philox(ST_INS, seg, attempt, idx = j, sub = c>>2).w[c&3]   (letters 16c..16c+15, c >= 1)
 * insertion letter i: 2-bit field (i&15) of its word; substitution letter i: the (i&15)-th base-3 digit of the
 * word read as a fraction (digit = (frac*3)>>32, frac = low 32 bits). */
static uint32_t payload_word(nso_draw *d, uint32_t seg, uint32_t attempt, uint32_t j, uint32_t c) {
    uint32_t w[4];
    if (c == 0) { philox_at(d, ST_SUB, seg, attempt, j >> 2, 0, w); return w[j & 3]; }
    philox_at(d, ST_INS, seg, attempt, j, c >> 2, w);
    return w[c & 3];
}
/* S:1968-1972: uniform choice among BASES minus the current base */
static uint8_t mis_letter(uint8_t cur, nso_draw *d, uint32_t seg, uint32_t attempt, uint32_t j, uint32_t i) {
    uint32_t dg = 0;
    if (d->mode) dg = (uint32_t)(tape_u(d) * 3);
    else {
        uint32_t frac = payload_word(d, seg, attempt, j, i >> 4);
        for (uint32_t t = 0; t <= (i & 15); ++t) { uint64_t p = (uint64_t)frac * 3u; dg = (uint32_t)(p >> 32); frac = (uint32_t)p; }
    }
    int rc = base_rank(cur);
    int rk = (int)dg + ((int)dg >= rc ? 1 : 0);
    if (rc < 0) rk = (int)dg;               /* cannot happen after resolve_base */
    return (uint8_t)BASES[rk];
}
/* S:1990 */
static uint8_t ins_letter(nso_draw *d, uint32_t seg, uint32_t attempt, uint32_t j, uint32_t i) {
    uint32_t v;
    if (d->mode) v = (uint32_t)(tape_u(d) * 4);
    else v = (payload_word(d, seg, attempt, j, i >> 4) >> (2 * (i & 15))) & 3u;
    return (uint8_t)BASES[v];
}
static uint8_t ht_letter(nso_draw *d, uint32_t stream, uint32_t attempt, uint32_t i) {             /* S:1426-1427 */
    uint32_t w[4];
    philox_at(d, stream, 0, attempt, i >> 6, 0, w);
    return (uint8_t)BASES[(w[(i >> 4) & 3] >> (2 * (i & 15))) & 3u];
}
static uint8_t qual_value(const ns_model_tables *t, int cls, uint32_t h) {
    const uint32_t *thr = t->qual_thr[cls];
    uint32_t q = 0;
    for (uint32_t j = 0; j < NS_QUAL_LEVELS - 1; ++j) q += (h >= thr[j]);
    return (uint8_t)q;
}
static uint8_t qual_at(const ns_model_tables *t, int cls, nso_draw *d, uint32_t stream, uint32_t seg,
                       uint32_t attempt, uint64_t m) {
    uint32_t w[4];
    philox_at(d, stream, seg, attempt, (uint32_t)(m >> 3), 0, w);
    uint32_t h = (w[(m & 7) >> 1] >> (16 * (m & 1))) & 0xffffu;
    return qual_value(t, cls, h);
}

/* ------------------------------------------------------------------------------------------------
 * mutate_read (S:1919-2015) — without the -k filter (added by nso_hp_filter below)
 *   seg_in : case_convert()ed segment (ref_len bases);  events ascending as generated
 *   out    : mutated bases; cls: quality class of every emitted base (match/mis/ins)
 *   log    : error-log rows in the reference's (descending) order
 * Events are walked in DESCENDING key order like the reference so that tape replay pops the letter
 * draws in the same order; the output is assembled right-to-left.
 * ---------------------------------------------------------------------------------------------- */
typedef struct nso_logrow { uint32_t pos, len, type, ref_off, new_off; } nso_logrow;   /* offsets into `txt` */

int64_t nso_mutate_read(const uint8_t *seg_in, int64_t ref_len, const ns_event *ev, uint64_t n_ev, nso_draw *d,
                        uint32_t seg, uint32_t attempt, uint8_t *out, uint8_t *cls, int64_t out_cap,
                        nso_logrow *log, uint8_t *txt, uint64_t *txt_len) {
    /* output length */
    int64_t out_len = ref_len;
    for (uint64_t j = 0; j < n_ev; ++j) {
        if (NS_EV_TYPE(ev[j].info) == NS_INS) out_len += NS_EV_LEN(ev[j].info);
        else if (NS_EV_TYPE(ev[j].info) == NS_DEL) out_len -= NS_EV_LEN(ev[j].info);
    }
    if (out_len > out_cap || out_len < 0) return -1;
    int64_t w = out_len;                  /* write cursor (exclusive) */
    int64_t prev = ref_len;               /* S:1958 */
    uint64_t tl = 0, row = 0;
    for (uint64_t jj = n_ev; jj-- > 0;) {
        const ns_event *e = &ev[jj];
        int64_t key = e->pos, len = NS_EV_LEN(e->info);
        const int etype = (int)NS_EV_TYPE(e->info);
        int64_t err_end = (etype == NS_INS) ? key : key + len;
        /* match run after the error: read[err_end:prev] */
        for (int64_t x = prev - 1; x >= err_end; --x) { --w; out[w] = seg_in[x]; if (cls) cls[w] = NS_Q_MATCH; }
        if (log) { log[row].pos = (uint32_t)key; log[row].len = (uint32_t)len; log[row].type = (uint32_t)etype;
                   log[row].ref_off = (uint32_t)tl; }
        if (etype == NS_MIS) {
            uint8_t nb[4096];
            for (int64_t i = 0; i < len; ++i) nb[i] = mis_letter(seg_in[key + i], d, seg, attempt, (uint32_t)jj, (uint32_t)i);
            for (int64_t i = len - 1; i >= 0; --i) { --w; out[w] = nb[i]; if (cls) cls[w] = NS_Q_MIS; }
            if (txt) { memcpy(txt + tl, seg_in + key, (size_t)len); tl += (uint64_t)len;
                       if (log) log[row].new_off = (uint32_t)tl;
                       memcpy(txt + tl, nb, (size_t)len); tl += (uint64_t)len; }
        } else if (etype == NS_DEL) {
            if (txt) { memcpy(txt + tl, seg_in + key, (size_t)len); tl += (uint64_t)len;
                       if (log) log[row].new_off = (uint32_t)tl;
                       memset(txt + tl, '-', (size_t)len); tl += (uint64_t)len; }
        } else {
            uint8_t nb[4096];
            for (int64_t i = 0; i < len; ++i) nb[i] = ins_letter(d, seg, attempt, (uint32_t)jj, (uint32_t)i);
            for (int64_t i = len - 1; i >= 0; --i) { --w; out[w] = nb[i]; if (cls) cls[w] = NS_Q_INS; }
            if (txt) { memset(txt + tl, '-', (size_t)len); tl += (uint64_t)len;
                       if (log) log[row].new_off = (uint32_t)tl;
                       memcpy(txt + tl, nb, (size_t)len); tl += (uint64_t)len; }
        }
        prev = key;
        ++row;
    }
    for (int64_t x = prev - 1; x >= 0; --x) { --w; out[w] = seg_in[x]; if (cls) cls[w] = NS_Q_MATCH; }
    if (txt_len) *txt_len = tl;
    return (w == 0) ? out_len : -2;
}

/* ------------------------------------------------------------------------------------------------
 * -k: the homopolymer filter of mutate_read (S:1920-1947) and mutate_homo (S:618-705)
 * ---------------------------------------------------------------------------------------------- */
/* Branch counters of the -k stage (test infrastructure, like nso_edge_counts): what nso_mutate_homo and nso_hp_filter met since the last reset. */
enum { NSO_HP_RUNS = 0,           /* re-sampled runs (>= k bases of A, C, G or T) */
       NSO_HP_GROW = 1,           /* ... whose new size is above the old one */
       NSO_HP_GROW_15 = 2,        /* ... by more than 15 bases (several insertions of <= 15 letters at one position) */
       NSO_HP_SHRINK = 3,         /* ... whose new size is below the old one */
       NSO_HP_SHRINK_4095 = 4,    /* ... by more than NS_EV_LEN_MAX bases (the deletion is split) */
       NSO_HP_SIZE0 = 5,          /* runs re-sampled to size 0 (S:652-654: a negative draw counts as 0) */
       NSO_HP_L64 = 6,            /* runs of 64 bases or more */
       NSO_HP_L1024 = 7,          /* runs of 1024 bases or more */
       NSO_HP_L4096 = 8,          /* runs of more than NS_EV_LEN_MAX bases */
       NSO_HP_AT_START = 9,       /* runs that start at the first base of the segment */
       NSO_HP_AT_END = 10,        /* runs that end at the last base of the segment */
       NSO_HP_MIS2 = 11,          /* runs with two or more mismatches */
       NSO_HP_MIS_APPENDED = 12,  /* runs with a mismatch on an appended base */
       NSO_HP_MIS_MID_INS = 13,   /* runs whose FIRST mismatch is an appended base that is not letter 0 of a 15-letter insertion counted from the run's end */
       NSO_HP_EDITS3 = 14,        /* runs with more than 2 edits (deletions of <= NS_EV_LEN_MAX + kept mismatches + insertions of <= 15 letters) */
       NSO_HP_EDITS_MAX = 15,     /* the largest number of edits of one run (a maximum, not a count) */
       NSO_HP_TIE = 16,           /* draws exactly on n + 1/2 (round half to even decides) */
       NSO_HP_ADJACENT = 17,      /* re-sampled runs that start where the previous re-sampled run ended */
       NSO_HP_DROP_MIS = 18, NSO_HP_DROP_INS = 19, NSO_HP_DROP_DEL = 20,   /* filter: events dropped, by type */
       NSO_HP_KEEP_MIS = 21, NSO_HP_KEEP_INS = 22, NSO_HP_KEEP_DEL = 23,   /* filter: events kept, by type */
       NSO_HP_INS_KEY_BEFORE = 24,/* filter: an insertion dropped only because base pos - 1 is in a run (its float key pos - 1/2, S:1929-1937) */
       NSO_HP_INS_KEY_BEYOND = 25,/* filter: an insertion dropped only because a base in (pos, pos + len - 1] is in a run */
       NSO_HP_NEAR_END = 26,      /* filter: events tested within 16 bases of either end of the segment */
       NSO_HP_RUN_CUT = 27,       /* filter: events tested on a run that touches an end of the segment and has fewer than k bases (k > 2: at least 2) */
       NSO_HP_SHIFT_RANGE = 28,   /* pieces dropped because the cumulative shift of their homopolymer edits left the event record's shift field */
       NSO_HP_N = 32 };
static uint64_t nso_hp[NSO_HP_N];
/* attempts dropped because an event left the fields of the 8-byte event record (ns_batch_info.n_range_redraws of the engine) */
static uint64_t nso_range_redraws;
uint64_t nso_range_redraw_count(int reset) { uint64_t v = nso_range_redraws; if (reset) nso_range_redraws = 0; return v; }
void nso_hp_counts(uint64_t *out, int reset) {
    for (int i = 0; i < NSO_HP_N; ++i) { if (out) out[i] = nso_hp[i]; if (reset) nso_hp[i] = 0; }
}

/* is base x of the (converted) segment inside a run of >= k identical bases? */
static int in_hp_run(const uint8_t *seg, int64_t n, int64_t x, int64_t k) {
    if (x < 0 || x >= n) return 0;
    int64_t s = x, e = x + 1;
    while (s > 0 && seg[s - 1] == seg[x] && e - s < k) --s;
    while (e < n && seg[e] == seg[x] && e - s < k) ++e;
    if (e - s < k && (s == 0 || e == n) && e - s >= (k > 2 ? 2 : 1)) ++nso_hp[NSO_HP_RUN_CUT];
    return e - s >= k;
}
/* Drops every event whose interval [key, key+len) (float keys: pos for mis/del, pos-0.5 for ins) overlaps a
 * homopolymer [s,e) of the un-mutated segment: not (e <= key or key+len <= s)  (S:1929-1937).  In integers:
 * mis/del overlap iff some base in [pos, pos+len) is in a run; ins iff some base in [pos-1, pos+len-1] is.
 * Kept events are compacted in place with their shifts recomputed.  Returns the new count. */
uint64_t nso_hp_filter(const uint8_t *seg, int64_t ref_len, ns_event *ev, uint64_t n_ev, int64_t k, int64_t *shift_out) {
    uint64_t w = 0; int64_t shift = 0;
    for (uint64_t j = 0; j < n_ev; ++j) {
        int64_t pos = ev[j].pos, len = NS_EV_LEN(ev[j].info); int ty = (int)NS_EV_TYPE(ev[j].info);
        int64_t lo = ty == NS_INS ? pos - 1 : pos, hi = ty == NS_INS ? pos + len - 1 : pos + len - 1;
        int hit = 0, before = 0, at = 0, beyond = 0;
        if (lo < 16 || hi >= ref_len - 16) ++nso_hp[NSO_HP_NEAR_END];
        for (int64_t x = lo; x <= hi; ++x)
            if (in_hp_run(seg, ref_len, x, k)) { hit = 1; if (x < pos) before = 1; else if (x == pos) at = 1; else beyond = 1; }
        if (hit) {
            ++nso_hp[NSO_HP_DROP_MIS + ty];
            if (ty == NS_INS && before && !at && !beyond) ++nso_hp[NSO_HP_INS_KEY_BEFORE];
            if (ty == NS_INS && beyond && !at && !before) ++nso_hp[NSO_HP_INS_KEY_BEYOND];
            continue;
        }
        ++nso_hp[NSO_HP_KEEP_MIS + ty];
        ev[w].pos = (uint32_t)pos; ev[w].info = NS_EV_PACK(len, ty, shift);
        if (ty == NS_INS) shift += len; else if (ty == NS_DEL) shift -= len;
        ++w;
    }
    if (shift_out) *shift_out = shift;
    return w;
}

/* get_nd_par (hp:246-260): mu = predict_piecewise (hp:167-186), sigma = predict_lr (hp:204-209) */
static void hp_nd_par(const ns_model_tables *t, uint8_t base, int64_t len, double *mu, double *sigma) {
    const ns_hp_class *h = &t->hp[(base == 'A' || base == 'T') ? 0 : 1];
    double x = (double)len;
    double y = h->konst + h->alpha1 * x;
    for (uint32_t j = 0; j < h->n_breaks; ++j) {
        double dlt = x - h->breakpoint[j];
        y += h->beta[j] * (dlt > 0 ? dlt : 0.0);
    }
    *mu = y; *sigma = h->intercept + h->slope * x;
}
double nso_hp_mu(const ns_model_tables *t, uint8_t base, int64_t len) { double m, s; hp_nd_par(t, base, len, &m, &s); return m; }
double nso_hp_sigma(const ns_model_tables *t, uint8_t base, int64_t len) { double m, s; hp_nd_par(t, base, len, &m, &s); return s; }

/* new base x of the re-sampled run that starts at s (S:671-682): mismatch with prob hp_mis_rate (0 < p <= rate) to a uniform other
 * base.  Draws: p = Philox(ST_HPMIS, idx = s, sub = x >> 2).word[x & 3]; the other base from c = Philox(ST_HPMIS, idx = s,
 * sub = 0x80000000 | x).word[0] as j = (c' * 3) >> 32 in "ATCG" order — for a KEPT base c' is c with bit 0 replaced by "first mismatch
 * of the run" (that bit travels in the engine's event word), for an appended base c' = c. */
static uint8_t hp_base(const ns_model_tables *t, uint8_t base, nso_draw *d, uint32_t seg, uint32_t attempt, uint32_t s, uint32_t x,
                       int kept, int first, int *is_mis) {
    double p; uint32_t j = 0;
    if (d->mode) {
        p = tape_u(d);
        if (0 < p && p <= t->hp_mis_rate) {
            for (;;) { uint8_t nb = (uint8_t)BASES[(uint32_t)(tape_u(d) * 4)]; if (nb != base) { *is_mis = 1; return nb; } }
        }
        *is_mis = 0; return base;
    }
    uint32_t w[4]; philox_at(d, ST_HPMIS, seg, attempt, s, x >> 2, w);
    p = u32_to_p(w[x & 3u]);
    if (!(0 < p && p <= t->hp_mis_rate)) { *is_mis = 0; return base; }
    uint32_t c[4]; philox_at(d, ST_HPMIS, seg, attempt, s, 0x80000000u | x, c);
    uint32_t cw = c[0];
    if (kept) cw = (cw & ~1u) | (first ? 1u : 0u);
    j = (uint32_t)(((uint64_t)cw * 3u) >> 32);
    int rc = base_rank(base);
    *is_mis = 1;
    return (uint8_t)BASES[j + ((int)j >= rc ? 1u : 0u)];
}

/* mutate_homo (S:618-705) on one mutated aligned segment.
 *   in/in_c: bases and their quality classes (or NULL) before; out/out_c after; returns the new length (-1 if out_cap is too small,
 *   -2 if the cumulative length change leaves the shift field of the event record).
 *   A kept base keeps its class (S:688-690: a contraction drops the FIRST |diff| qualities of the run), an appended base is 'ins'
 *   (S:692-695), the first mismatch of a run 'mis' (S:697-700).  The qualities themselves are drawn afterwards, by final position.
 *   Draw keys: new length of the run starting at s: ST_HPLEN idx=s; new base x of the run: hp_base. */
int64_t nso_mutate_homo(const ns_model_tables *t, const uint8_t *in, const uint8_t *in_c, int64_t n, int64_t k, nso_draw *d,
                        uint32_t seg, uint32_t attempt, uint8_t *out, uint8_t *out_c, int64_t out_cap) {
    int64_t w = 0, p = 0, prev_end = -1;
    while (p < n) {
        int64_t s = p, e = p + 1;
        while (e < n && in[e] == in[s]) ++e;
        const int64_t L = e - s;
        const uint8_t b = in[s];
        if (L < k || base_rank(b) < 0) {
            if (w + L > out_cap) return -1;
            memcpy(out + w, in + s, (size_t)L);
            if (in_c) memcpy(out_c + w, in_c + s, (size_t)L);
            w += L; p = e;
            continue;
        }
        double mu, sigma, x;
        hp_nd_par(t, b, L, &mu, &sigma);
        if (d->mode) x = tape_z(d);                                   /* np.random.normal(mu, sigma) recorded from the reference */
        else { uint32_t ww[4]; philox_at(d, ST_HPLEN, seg, attempt, (uint32_t)s, 0, ww); x = fma(sigma, nso_norminv(u32_to_p(ww[0])), mu); }
        if (x < 0) x = 0;                                             /* S:652-654 */
        const int64_t size = nso_f64_to_i64_sat(nearbyint(x));        /* int(round(.)), S:665 */
        /* the engine files the run's edits as 8-byte event records that carry the piece's cumulative length change so far in an 18-bit
         * field: a piece whose change leaves that field behind any of its runs is dropped with its attempt, like a
         * chain event that does not fit */
        if (size - L >= 2 * (int64_t)NS_EV_SHIFT_BIAS || w + size - e < -(int64_t)NS_EV_SHIFT_BIAS || w + size - e >= (int64_t)NS_EV_SHIFT_BIAS) {
            ++nso_hp[NSO_HP_SHIFT_RANGE]; return -2;
        }
        if (w + size > out_cap) return -1;
        int64_t first_mis = -1, n_mis = 0, n_kept_mis = 0, n_ins = 0, cnt = 0;
        int mis_app = 0, mid_ins = 0;
        for (int64_t i = 0; i < size; ++i) {
            int is_mis; uint8_t nb;
            const int kept = (size <= L || i < L);
            nb = hp_base(t, b, d, seg, attempt, (uint32_t)s, (uint32_t)i, kept, first_mis < 0, &is_mis);
            if (in_c) {
                if (kept) out_c[w + i] = in_c[(size <= L) ? s + (L - size) + i : s + i];   /* kept position (S:688-690: the first |diff| quals go) */
                else out_c[w + i] = (uint8_t)NS_Q_INS;                                        /* appended base (S:692-695) */
            }
            out[w + i] = nb;
            if (!kept) {                                              /* (counters) appended bases travel as insertions of <= 15 letters; the */
                if (is_mis && first_mis < 0 && cnt) { ++n_ins; cnt = 0; mid_ins = 1; }   /* run's first mismatch opens its own */
                if (++cnt == 15) { ++n_ins; cnt = 0; }
                if (is_mis) mis_app = 1;
            } else if (is_mis) ++n_kept_mis;
            if (is_mis) ++n_mis;
            if (is_mis && first_mis < 0) first_mis = i;
        }
        if (cnt) ++n_ins;
        if (in_c && first_mis >= 0) out_c[w + first_mis] = (uint8_t)NS_Q_MIS;               /* S:697-700 */
        {
            const int64_t edits = (size < L ? (L - size + NS_EV_LEN_MAX - 1) / NS_EV_LEN_MAX : 0) + n_kept_mis + n_ins;
            ++nso_hp[NSO_HP_RUNS];
            if (size > L) ++nso_hp[NSO_HP_GROW];
            if (size > L + 15) ++nso_hp[NSO_HP_GROW_15];
            if (size < L) ++nso_hp[NSO_HP_SHRINK];
            if (L - size > (int64_t)NS_EV_LEN_MAX) ++nso_hp[NSO_HP_SHRINK_4095];
            if (size == 0) ++nso_hp[NSO_HP_SIZE0];
            if (L >= 64) ++nso_hp[NSO_HP_L64];
            if (L >= 1024) ++nso_hp[NSO_HP_L1024];
            if (L > (int64_t)NS_EV_LEN_MAX) ++nso_hp[NSO_HP_L4096];
            if (s == 0) ++nso_hp[NSO_HP_AT_START];
            if (e == n) ++nso_hp[NSO_HP_AT_END];
            if (n_mis >= 2) ++nso_hp[NSO_HP_MIS2];
            if (mis_app) ++nso_hp[NSO_HP_MIS_APPENDED];
            if (mid_ins) ++nso_hp[NSO_HP_MIS_MID_INS];
            if (edits > 2) ++nso_hp[NSO_HP_EDITS3];
            if ((uint64_t)edits > nso_hp[NSO_HP_EDITS_MAX]) nso_hp[NSO_HP_EDITS_MAX] = (uint64_t)edits;
            if (x - floor(x) == 0.5) ++nso_hp[NSO_HP_TIE];
            if (s == prev_end) ++nso_hp[NSO_HP_ADJACENT];
            prev_end = e;
        }
        w += size; p = e;
    }
    return w;
}

/* ------------------------------------------------------------------------------------------------
 * lengths, positions
 * ---------------------------------------------------------------------------------------------- */
/* KernelDensity.sample (sklearn, call site S:235): i = floor(U*n); x = N(data[i], bw) */
static double kde_sample(const ns_kde *k, const uint32_t w[4]) {
    uint64_t i = (uint64_t)(u53_to_p(w[0], w[1]) * (double)k->n);
    if (i >= k->n) i = k->n - 1;
    return fma(k->bw, nso_norminv(u32_to_p(w[2])), k->data[i]);
}
static double pow10m1(double x) { return nso_exp(x * 2.302585092994046) - 1.0; }   /* S:236-237 */

/* extract_read, genome branches (S:1750-1781).  Returns 0 and fills chrom/pos on success. */
static int extract_pos(const uint64_t *chrom_off, uint32_t nchrom, const uint8_t *circular, int64_t length,
                       nso_draw *d, uint32_t seg, uint32_t attempt, uint32_t *chrom, uint64_t *pos) {
    uint64_t genome_len = chrom_off[nchrom];
    for (uint32_t j = 0; j < NSO_POS_RETRY; ++j) {
        uint32_t w[4];
        philox_at(d, ST_POS, seg, attempt, j, 0, w);
        uint64_t ref_pos = (uint64_t)(u53_to_p(w[0], w[1]) * (double)(genome_len + 1));   /* randint(0, genome_len) */
        if (ref_pos > genome_len) ref_pos = genome_len;
        if (circular[0]) {                       /* S:1752-1760: first chromosome, wrap-around */
            *chrom = 0; *pos = ref_pos; return 0;
        }
        for (uint32_t c = 0; c < nchrom; ++c) {  /* S:1770-1778 */
            uint64_t cl = chrom_off[c + 1] - chrom_off[c];
            if (ref_pos + (uint64_t)length <= cl) {
                if (length == 0) { *chrom = c; *pos = ref_pos; return 0; }    /* the reference would spin here */
                *chrom = c; *pos = ref_pos; return 0;
            } else if (ref_pos < cl) break;
            else ref_pos -= cl;
        }
    }
    return -1;
}

/* ------------------------------------------------------------------------------------------------
 * whole-read restatement: simulation_aligned_genome (S:1266-1454), simulation_unaligned (S:1482-1549),
 * simulation_gap (S:1552-1568)
 * ---------------------------------------------------------------------------------------------- */
typedef struct nso_ref {
    const uint8_t *bases;            /* normalised (upper-case, IUPAC) */
    const uint64_t *chrom_off;
    uint32_t nchrom;
    const uint8_t *circular;
    const char *const *names;
} nso_ref;

typedef struct nso_out {
    ns_read *reads; ns_piece *pieces; ns_event *events;
    uint64_t cap_pieces, cap_events;
    uint8_t *records; uint64_t cap_records;
    uint8_t *errlog; uint64_t cap_errlog;
    uint64_t n_pieces, n_events, record_bytes, errlog_bytes, total_bases, total_ref_bases;
    uint16_t *polya;                 /* transcriptome: polyA tail length per read (may be NULL) */
    uint8_t *spliced; uint64_t cap_spliced, spliced_bytes;   /* intron retention: the spliced stretches (may be NULL) */
} nso_out;

#define NSO_MAX_SEG 64

/* ================================================================================================
 * metagenome mode
 * ============================================================================================== */
enum { ST_SPECIES = 21 };

typedef struct nso_meta {            /* species view of the reference (src/simulator.py:284-339) */
    uint32_t nspecies;
    const uint32_t *species_chrom_off;   /* [nspecies+1] */
    const double *abun;                  /* dict_abun, in species order */
    const double *abun_inflated;         /* dict_abun_inflated (chimeric) or NULL */
} nso_meta;

/* assign_species (S:758-811).  lengths/segs are the pass's filtered length list and remaining segment counts;
 * out_species/out_lengths get one entry per assigned segment, out_segs the sorted segment counts.  Returns the number of
 * assigned segments.  Draws: tape (u for random.choice -> floor(u*n); random.uniform(0,100) -> 100*u) or Philox keyed
 * (ST_SPECIES, attempt = pass, idx = segment pointer): word 0 = choice, word 1 = uniform. */
static int cmp_desc_d(const void *a, const void *b) { double x = *(const double *)a, y = *(const double *)b; return x < y ? 1 : x > y ? -1 : 0; }
static int cmp_desc_i(const void *a, const void *b) { int32_t x = *(const int32_t *)a, y = *(const int32_t *)b; return x < y ? 1 : x > y ? -1 : 0; }

uint64_t nso_assign_species(const nso_meta *mg, const double *lengths, uint64_t n_len, const int32_t *segs, uint64_t n_reads,
                            const double *current_bases, nso_draw *d, uint32_t pass, uint16_t *out_species, double *out_lengths,
                            int32_t *out_segs) {
    const uint32_t ns = mg->nspecies;
    memcpy(out_segs, segs, sizeof(int32_t) * n_reads);
    qsort(out_segs, n_reads, sizeof(int32_t), cmp_desc_i);                      /* S:760 */
    uint64_t segs_chimera = 0;
    for (uint64_t i = 0; i < n_reads; ++i) if (segs[i] > 1) segs_chimera += (uint64_t)segs[i];   /* S:761 */
    if (segs_chimera > n_len) segs_chimera = n_len;
    memcpy(out_lengths, lengths, sizeof(double) * n_len);
    qsort(out_lengths + segs_chimera, n_len - segs_chimera, sizeof(double), cmp_desc_d);          /* S:764-765 */
    double bases_to_add = 0;
    for (uint64_t i = 0; i < n_len; ++i) bases_to_add += lengths[i];             /* sum(length_list), left to right */
    double cur_total = 0, total_abun = 0;
    for (uint32_t s = 0; s < ns; ++s) { cur_total += current_bases[s]; total_abun += mg->abun[s]; }
    const double total_bases = bases_to_add + cur_total;
    double quota[256];
    for (uint32_t s = 0; s < ns; ++s) quota[s] = total_bases * mg->abun[s] / total_abun - current_bases[s];   /* S:772-775 */
    uint64_t ptr = 0;
    uint32_t pre = 0;
    uint32_t avail[256];
    for (uint64_t r = 0; r < n_reads; ++r) {
        const int32_t seg = out_segs[r];
        if (ptr + (uint64_t)seg > n_len) break;                                  /* S:781-782 */
        for (int32_t each = 0; each < seg; ++each) {
            const double len = out_lengths[ptr];
            uint32_t w[4] = {0, 0, 0, 0};
            if (!d->mode) {
                uint32_t c3 = (ST_SPECIES & 0x3fu) << 18 | (pass & 0x3ffu);
                nso_philox((uint32_t)d->seed, (uint32_t)(d->seed >> 32), (uint32_t)ptr, (uint32_t)(ptr >> 32), (uint32_t)d->read,
                           c3 | (uint32_t)((d->read >> 32) & 0xffu) << 24, w);
            }
            uint32_t sp = 0, n = 0;
#define NSO_CHOOSE() (d->mode ? avail[(uint32_t)(tape_u(d) * n)] : avail[(uint32_t)(((uint64_t)w[0] * n) >> 32)])
            if (each == 0) {
                for (uint32_t s = 0; s < ns; ++s) if (quota[s] - len > 0) avail[n++] = s;          /* S:785-788 */
                if (!n) for (uint32_t s = 0; s < ns; ++s) if (quota[s] > 0) avail[n++] = s;
                if (!n) return ptr;                     /* random.choice([]) raises in the reference */
                sp = NSO_CHOOSE();
            } else {
                for (uint32_t s = 0; s < ns; ++s) if (quota[s] - len > 0 && s != pre) avail[n++] = s;   /* S:791-792 */
                const double p = d->mode ? 100.0 * tape_u(d) : 100.0 * u32_to_p(w[1]);                /* S:793 */
                if (p <= mg->abun_inflated[pre] && quota[pre] > 0) sp = pre;
                else if (p > mg->abun_inflated[pre] && n > 0) sp = NSO_CHOOSE();
                else {
                    n = 0;
                    for (uint32_t s = 0; s < ns; ++s) if (quota[s] - len > 0) avail[n++] = s;
                    if (!n) for (uint32_t s = 0; s < ns; ++s) if (quota[s] > 0) avail[n++] = s;
                    if (!n) return ptr;
                    sp = NSO_CHOOSE();
                }
            }
            out_species[ptr] = (uint16_t)sp;
            quota[sp] -= len;
            ++ptr;
            pre = sp;
        }
    }
    return ptr;
}

/* extract_read, metagenome branch (S:1704-1749).  species < 0: random species (S:1705-1706).  Returns 0 and the global
 * chromosome index + start, 1 additionally when another species had to be used (the reference prints a warning), <0 if no
 * chromosome is long enough (assert at S:1726).
 * Draws: tape (choice -> floor(u*n), randint(a,b) -> a + floor(u*(b-a+1))) or Philox (ST_POS, seg, attempt): block idx 0:
 * word 0 species, word 1 chromosome, word 2 fallback choice; block idx 1: 53-bit position. */
int nso_extract_meta(const nso_meta *mg, const uint64_t *chrom_off, const uint8_t *circular, int64_t length, int species,
                     nso_draw *d, uint32_t seg, uint32_t attempt, uint32_t *chrom, uint64_t *pos) {
    uint32_t wa[4] = {0, 0, 0, 0}, wb[4] = {0, 0, 0, 0};
    if (!d->mode) { philox_at(d, ST_POS, seg, attempt, 0, 0, wa); philox_at(d, ST_POS, seg, attempt, 1, 0, wb); }
    int warned = 0;
    uint32_t s;
    if (species < 0) s = d->mode ? (uint32_t)(tape_u(d) * mg->nspecies) : (uint32_t)(((uint64_t)wa[0] * mg->nspecies) >> 32);
    else s = (uint32_t)species;
    uint32_t nch = mg->species_chrom_off[s + 1] - mg->species_chrom_off[s];
    uint32_t c = mg->species_chrom_off[s] + (d->mode ? (uint32_t)(tape_u(d) * nch) : (uint32_t)(((uint64_t)wa[1] * nch) >> 32));
    uint64_t clen = chrom_off[c + 1] - chrom_off[c];
    if ((uint64_t)length > clen) {                                               /* S:1711-1735 */
        uint32_t total = mg->species_chrom_off[mg->nspecies];
        uint32_t *target = (uint32_t *)malloc(sizeof(uint32_t) * (total + 1)), *other = (uint32_t *)malloc(sizeof(uint32_t) * (total + 1));
        uint32_t nt = 0, no = 0;
        for (uint32_t ts = 0; ts < mg->nspecies; ++ts)
            for (uint32_t k = mg->species_chrom_off[ts]; k < mg->species_chrom_off[ts + 1]; ++k)
                if ((uint64_t)length < chrom_off[k + 1] - chrom_off[k]) { if (ts == s) target[nt++] = k; else other[no++] = k; }
        if (!nt && !no) { free(target); free(other); return -1; }
        if (nt) c = target[d->mode ? (uint32_t)(tape_u(d) * nt) : (uint32_t)(((uint64_t)wa[2] * nt) >> 32)];
        else { c = other[d->mode ? (uint32_t)(tape_u(d) * no) : (uint32_t)(((uint64_t)wa[2] * no) >> 32)]; warned = 1; }
        free(target); free(other);
        clen = chrom_off[c + 1] - chrom_off[c];
    }
    uint64_t span = circular[c] ? clen + 1 : clen - (uint64_t)length + 1;        /* randint(0, len) / randint(0, len - length) */
    uint64_t rp = d->mode ? (uint64_t)(tape_u(d) * (double)span) : (uint64_t)(u53_to_p(wb[0], wb[1]) * (double)span);
    if (rp >= span) rp = span - 1;
    *chrom = c; *pos = rp;
    return warned;
}

/* ================================================================================================
 * transcriptome mode
 * ============================================================================================== */
enum { ST_TRX = 22, ST_IR = 23 };

typedef struct nso_trx {             /* expression view of the reference transcripts (src/simulator.py:382-399, 460-470) */
    uint32_t n_expr;
    const uint32_t *expr_chrom;          /* transcripts with TPM > 0 in the order of make_cdf (S:69-97) */
    const double *expr_cum;              /* running sum of ecdf_weight_list, as random.choices accumulates it (S:1084) */
    const uint8_t *polya;                /* [nchrom] 1 = listed in --polya, or NULL */
    double polya_scale;                  /* S:1046-1049 */
    const ns_ir_tables *ir;              /* intron retention (S:403-452) or NULL */
} nso_trx;

/* ---- intron retention ---------------------------------------------------------------------------
 * PARITY: nso_ir_states is pinned against the reference's update_structure and nso_extract_read_pos against its extract_read_pos
 * (tests/golden/reference_ir.json: 400 + 496 recorded calls; HTSeq.GenomicInterval, which extract_read_pos only constructs, is a
 * four-field record in the fixture generator).  The splice (nso_splice) is restated from S:1159-1178 and pinned the same way (it was UNPINNED until round 3): the reference fetches
 * the intervals through pysam, which this image lacks. */

/* update_structure (S:114-145): u[k] is the random.random() of intron k; retained[k] = 1 for "IR".  Returns flag_ir.
 * (A p beyond both intervals of the row — its two probabilities summing to less than 1 — appends nothing in the reference, which
 * then runs out of list_states; it counts as no_IR here.) */
int nso_ir_states(const ns_ir_tables *t, uint32_t trx, const double *u, uint8_t *retained) {
    int prev = 0, flag = 0;
    uint32_t k = 0;
    for (uint32_t i = t->item_off[trx]; i < t->item_off[trx + 1]; ++i) {
        if (t->item_type[i] != NS_IR_INTRON) continue;
        const double p = u[k];
        if (0 <= p && p < t->p_no_ir[prev]) { retained[k] = 0; prev = 1; }
        else if (t->p_no_ir[prev] <= p && p < t->p_no_ir[prev] + t->p_ir[prev]) { retained[k] = 1; prev = 2; flag = 1; }
        else { retained[k] = 0; prev = 1; }
        ++k;
    }
    return flag;
}

typedef struct nso_iv { uint32_t chrom, start, end; uint8_t retained, minus; } nso_iv;

/* The splice of the transcriptome worker (S:1161-1178): genome_fai.fetch(chrom, start, end) of every interval extract_read_pos returned,
 * concatenated, and reverse_complement (S:1675-1680: upper-case A, C, G, T only; everything else stays) when the LAST interval is on
 * strand '-'.  The bases are the file's (case kept; the device form is applied by the caller).  Returns the length, -1 if it exceeds cap.
 * PARITY: pinned against the reference's worker run with a FASTA record in place of pysam.Fastafile (tests/golden/reference_ir_splice.json). */
int64_t nso_splice(const ns_ir_tables *t, const nso_iv *iv, int n, uint8_t *out, int64_t cap) {
    int64_t got = 0;
    for (int z = 0; z < n; ++z)
        for (uint32_t x = iv[z].start; x < iv[z].end; ++x) {
            if (got >= cap) return -1;
            out[got++] = t->genome[t->genome_off[iv[z].chrom] + x];
        }
    if (n > 0 && iv[n - 1].minus) {
        for (int64_t i = 0, j = got - 1; i <= j; ++i, --j) {
            uint8_t x = out[i], y = out[j];
            uint8_t cx = x == 'A' ? 'T' : x == 'T' ? 'A' : x == 'C' ? 'G' : x == 'G' ? 'C' : x;
            uint8_t cy = y == 'A' ? 'T' : y == 'T' ? 'A' : y == 'C' ? 'G' : y == 'G' ? 'C' : y;
            out[i] = cy; out[j] = cx;
        }
    }
    return got;
}

/* extract_read_pos (S:148-191) on the structure with the introns of `retained` switched to "retained_intron"; u_start is the
 * uniform behind random.randint(0, min(ref_len - length, len_before)).  Returns the number of intervals (list_intervals). */
int nso_extract_read_pos(const ns_ir_tables *t, uint32_t trx, const uint8_t *retained, int64_t length, int64_t ref_len, double u_start,
                         int polya, nso_iv *iv, uint32_t cap, int *retain_polya) {
    const uint32_t i0 = t->item_off[trx], i1 = t->item_off[trx + 1];
    int64_t len_before = 0;
    uint32_t k = 0;
    for (uint32_t i = i0; i < i1; ++i) {                                   /* S:153-159 */
        if (t->item_type[i] == NS_IR_EXON) len_before += t->item_len[i];
        else if (retained[k++]) break;
    }
    int64_t hi = ref_len - length < len_before ? ref_len - length : len_before;
    int64_t start_pos = (int64_t)(u_start * (double)(hi + 1));
    if (start_pos > hi) start_pos = hi;
    uint32_t n = 0;
    int64_t end = 0;
    k = 0;
    for (uint32_t i = i0; i < i1; ++i) {                                   /* S:164-184 */
        if (length == 0) break;
        int is_ret = 0;
        if (t->item_type[i] == NS_IR_INTRON) { is_ret = retained[k++]; if (!is_ret) continue; }
        const int64_t ilen = t->item_len[i], istart = t->item_start[i], iend = istart + ilen;
        if (start_pos < ilen) {
            const int64_t start = start_pos + istart;
            end = start + length <= iend ? start + length : iend;
            length -= end - start;
            start_pos = 0;
            if (n >= cap) return -1;
            iv[n].chrom = t->item_chrom[i]; iv[n].start = (uint32_t)start; iv[n].end = (uint32_t)end;
            iv[n].retained = (uint8_t)is_ret; iv[n].minus = t->item_minus[i];
            ++n;
        } else start_pos -= ilen;
    }
    *retain_polya = polya && n && end + 10 >= (int64_t)t->item_start[i1 - 1] + (int64_t)t->item_len[i1 - 1];   /* S:186-189 */
    return (int)n;
}

/* random.choices(population, weights): bisect_right(cum_weights, random() * total, 0, n - 1) */
uint32_t nso_trx_pick(const nso_trx *tx, double u) {
    const double v = u * tx->expr_cum[tx->n_expr - 1];
    uint32_t lo = 0, hi = tx->n_expr - 1;
    while (lo < hi) { uint32_t mid = (lo + hi) >> 1; if (v < tx->expr_cum[mid]) hi = mid; else lo = mid + 1; }
    return lo;
}

/* select_nearest_kde2d (S:108-111) on a fresh, large sample of the 2-D KDE == a draw of the aligned length from the KDE
 * conditioned on the transcript length L: training point i with probability proportional to exp(-(L - x_i)^2 / 2h^2), then
 * y = y_i + h * N(0,1), int() truncation.  Rejection sampling inside the window |x_i - L| <= 5h; without a training point in the
 * window: the nearest one.  Draws: Philox (ST_REFLEN, seg 0, attempt, idx = try, sub). */
int64_t nso_kde2d_cond(const ns_model_tables *t, double L, nso_draw *d, uint32_t attempt, uint32_t sub) {
    const double *x = t->kde2d_x, *y = t->kde2d_y, h = t->kde2d_bw;
    const uint64_t n = t->kde2d_n;
    uint64_t lo = 0, hi = n;
    { uint64_t a = 0, b = n; const double v = L - 5.0 * h; while (a < b) { uint64_t m = (a + b) >> 1; if (x[m] < v) a = m + 1; else b = m; } lo = a; }
    { uint64_t a = lo, b = n; const double v = L + 5.0 * h; while (a < b) { uint64_t m = (a + b) >> 1; if (x[m] <= v) a = m + 1; else b = m; } hi = a; }
    uint32_t w[4];
    if (hi > lo) {
        for (uint32_t j = 0; j < NSO_KDE_RETRY; ++j) {
            philox_at(d, ST_REFLEN, 0, attempt, j, sub, w);
            uint64_t i = lo + (uint64_t)(u53_to_p(w[0], w[1]) * (double)(hi - lo));
            if (i >= hi) i = hi - 1;
            const double dd = (L - x[i]) / h;
            if (u32_to_p(w[2]) <= nso_exp(-0.5 * dd * dd)) return nso_f64_to_i64_sat(fma(h, nso_norminv(u32_to_p(w[3])), y[i]));
        }
    }
    uint64_t a = 0, b = n;
    while (a < b) { uint64_t m = (a + b) >> 1; if (x[m] < L) a = m + 1; else b = m; }
    uint64_t i = a >= n ? n - 1 : a;
    if (a > 0 && a < n && L - x[a - 1] <= x[a] - L) i = a - 1;
    philox_at(d, ST_REFLEN, 0, attempt, NSO_KDE_RETRY, sub, w);
    return nso_f64_to_i64_sat(fma(h, nso_norminv(u32_to_p(w[3])), y[i]));
}

/* extract_read("transcriptome", length) (S:1695-1703): a uniformly drawn transcript that is longer than the read, uniform start */
static int extract_trx_unaligned(const uint64_t *chrom_off, uint32_t nchrom, int64_t length, nso_draw *d, uint32_t seg, uint32_t attempt,
                                 uint32_t *chrom, uint64_t *pos) {
    uint32_t w[4];
    for (uint32_t j = 0; j < NSO_POS_RETRY; ++j) {
        philox_at(d, ST_POS, seg, attempt, j, 0, w);
        uint32_t c = (uint32_t)(((uint64_t)w[0] * nchrom) >> 32);
        uint64_t cl = chrom_off[c + 1] - chrom_off[c];
        if ((uint64_t)length < cl) {
            uint64_t span = cl - (uint64_t)length + 1, rp = (uint64_t)(u53_to_p(w[1], w[2]) * (double)span);
            if (rp >= span) rp = span - 1;
            *chrom = c; *pos = rp;
            return 0;
        }
    }
    return -1;
}

/* one read of a metagenome pass: lengths / species come from assign_species, the strand from the pass (S:860) */
typedef struct nso_mread {
    uint32_t pass, nseg, pos_in_pass, reversed;
    uint64_t seq_index;                 /* number of the read = reads accepted before it (S:909-911) */
    const int64_t *ref_len;             /* int(round(.)) of the assigned lengths, S:871 */
    const uint16_t *species;
} nso_mread;

/* one CANDIDATE read of a transcriptome block (trx_block below): transcript and aligned length come from the block's pick walk, every
 * other draw of the read is keyed by the candidate (key read index, attempt); one try — a candidate that fails is dropped */
typedef struct nso_tread {
    uint64_t key_read;                  /* absolute read index of the Philox key */
    uint32_t attempt;
    uint32_t chrom;                     /* the transcript */
    int64_t ref_len;                    /* ref_len_aligned (S:1098-1104) */
    uint64_t seq_index;                 /* slot of the read in the batch = its number - first_read */
} nso_tread;

static void fetch_segment(const nso_ref *ref, uint32_t chrom, uint64_t pos, int64_t len, uint8_t *dst) {
    uint64_t c0 = ref->chrom_off[chrom], cl = ref->chrom_off[chrom + 1] - c0;
    for (int64_t i = 0; i < len; ++i) {
        uint64_t x = pos + (uint64_t)i;
        if (x >= cl) x -= cl;                      /* circular wrap (S:1757-1760); never taken for linear */
        dst[i] = ref->bases[c0 + x];
    }
}

static int u64_digits(uint64_t v, char *buf) { return sprintf(buf, "%llu", (unsigned long long)v); }

/* Generates read `index` of the batch.  Returns 0, or <0 if buffers are too small / attempts exhausted. */
static int gen_read(const ns_model_tables *t, const nso_ref *ref, const ns_params *prm, uint64_t index, nso_out *o,
                    const nso_mread *mr, const nso_meta *mg, const nso_trx *tx, const nso_tread *tr) {
    nso_draw d; memset(&d, 0, sizeof d);
    d.mode = 0; d.seed = prm->seed; d.read = tr ? tr->key_read : prm->first_read + (mr ? mr->pos_in_pass : index);
    if (mr) index = mr->seq_index;
    if (tr) index = tr->seq_index;
    uint32_t w[4];
    const int kind = (int)prm->kind;
    uint32_t nseg = 1;
    if (mr) nseg = mr->nseg;
    uint32_t epoch = 0, fails = 0;
    uint32_t trx_chrom = 0; int64_t trx_len = 0;
    for (uint32_t a = mr ? mr->pass : tr ? tr->attempt : 0; a < NSO_MAX_ATTEMPT; ++a) {
        int64_t ref_len[NSO_MAX_SEG], gap_len[NSO_MAX_SEG];
        int ok = 1;
        if (!mr && kind == NS_KIND_ALIGNED && prm->chimeric) {
            /* S:1276-1277.  The reference draws num_segment once per worker and hands the segment counts out by POSITION among the
             * reads still missing (remaining_segments = num_segment[passed:], S:1447): a count that no draw of lengths can satisfy is
             * not retried for ever, the next while-iteration pairs the slot with other counts.  Here the count belongs to the epoch
             * of the read: it is drawn again whenever the read draws new lengths. */
            philox_at(&d, ST_NSEG, 0, epoch, 0, 0, w);
            nseg = (uint32_t)table_value(t->nseg_cdf, t->nseg_n, u32_to_p(w[0]));
            if (nseg > NSO_MAX_SEG) nseg = NSO_MAX_SEG;
        }
        if (mr && a != mr->pass) return 1;          /* metagenome: one try per pass; a rejected read is re-planned */
        if (tr && a != tr->attempt) return 1;       /* transcriptome: one try per candidate of the block's pick walk */
        /* ---- lengths ---- */
        if (kind == NS_KIND_UNALIGNED) {                                  /* S:1494-1495,1499 */
            philox_at(&d, ST_ULEN, 0, a, 0, 0, w);
            double x = prm->use_lognormal ? nso_exp(fma(prm->sd_len, nso_norminv(u32_to_p(w[2])), nso_log(prm->median_len)))
                                          : kde_sample(&t->kde[NS_KDE_UNALIGNED], w);
            ref_len[0] = len_draw(x);                                     /* above max_len: -1, rejected below unwalked */
            if (ref_len[0] > prm->max_len) ref_len[0] = -1;
            if (ref_len[0] < 0 && x > 0) ++nso_edges[NSO_EDGE_ULEN_LONG];
            if (x >= 2147483648.0) ++nso_edges[NSO_EDGE_ULEN_HUGE];
        } else if (tx) {                                                  /* transcriptome, S:1082-1105: planned by trx_block */
            if (!tr) return -40;
            trx_chrom = tr->chrom;
            trx_len = (int64_t)(ref->chrom_off[trx_chrom + 1] - ref->chrom_off[trx_chrom]);
            ref_len[0] = tr->ref_len;
        } else if (mr) {                                                  /* S:871-872 (aligned and --perfect) */
            for (uint32_t s = 0; s < nseg; ++s) ref_len[s] = mr->ref_len[s];
            for (uint32_t g = 0; g + 1 < nseg; ++g) {
                philox_at(&d, ST_GAPLEN, g, a, 0, 0, w);
                double x = pow10m1(kde_sample(&t->kde[NS_KDE_GAP], w));
                int64_t gi = nso_f64_to_i64_sat(x); gap_len[g] = gi < 0 ? 0 : gi;
            }
        } else {
            for (uint32_t s = 0; s < nseg && ok; ++s) {                   /* S:1285-1296,1309 */
                uint32_t j = 0;
                for (; j < NSO_KDE_RETRY; ++j) {
                    philox_at(&d, ST_REFLEN, s, epoch, j, 0, w);
                    double x;
                    if (!prm->use_lognormal) x = kde_sample(&t->kde[NS_KDE_ALIGNED], w);
                    else if (kind == NS_KIND_PERFECT)                      /* S:1286-1287 */
                        x = nso_exp(fma(prm->sd_len, nso_norminv(u32_to_p(w[2])), nso_log(prm->median_len)));
                    else {                                                 /* S:1293-1295 */
                        uint32_t w2[4];
                        philox_at(&d, ST_REFLEN, s, epoch, j, 1, w2);
                        double tot = nso_exp(fma(prm->sd_len, nso_norminv(u32_to_p(w[2])),
                                                 nso_log(prm->median_len + prm->sd_len * prm->sd_len / 2)));
                        double rem = pow10m1(kde_sample(&t->kde[NS_KDE_HT], w2));
                        if (rem < 0) continue;
                        x = tot - rem;
                    }
                    if (x >= 2147483648.0) ++nso_edges[NSO_EDGE_LEN_HUGE];
                    int keep = (kind == NS_KIND_PERFECT) ? ((double)prm->min_len <= x && x <= (double)prm->max_len)
                                                         : (0 < x && x <= (double)prm->max_len);
                    if (keep) { ref_len[s] = (int64_t)x; break; }
                }
                if (j == NSO_KDE_RETRY) ok = 0;
            }
            for (uint32_t g = 0; g + 1 < nseg; ++g) {                      /* S:1298-1299 */
                philox_at(&d, ST_GAPLEN, g, epoch, 0, 0, w);
                double x = pow10m1(kde_sample(&t->kde[NS_KDE_GAP], w));
                int64_t gi = nso_f64_to_i64_sat(x); gap_len[g] = gi < 0 ? 0 : gi;
            }
        }
        int64_t remainder = 0; double ratio = 0; int reversed;
        if (tx && kind == NS_KIND_ALIGNED) {                               /* S:1073-1076, 1203-1204: one draw per read, no filter */
            philox_at(&d, ST_HT, 0, a, 0, 0, w);
            double x = pow10m1(kde_sample(&t->kde[NS_KDE_HT], w));
            remainder = nso_f64_to_i64_sat(x);                             /* int(): towards zero */
            if (x >= 2147483648.0) ++nso_edges[NSO_EDGE_REM_HUGE];
            if (remainder < 0) remainder = 0;
            if (remainder > NSO_LEN_DRAW_MAX) { remainder = NSO_LEN_DRAW_MAX; ++nso_edges[NSO_EDGE_REM_SAT]; }
            philox_at(&d, ST_RATIO, 0, a, 0, 0, w);
            ratio = kde_sample(&t->kde[NS_KDE_RATIO], w);
            if (ratio > 1) ratio = 1;
            if (ratio < 0) ratio = 0;
        } else
        if (kind == NS_KIND_ALIGNED && ok) {                               /* S:1471-1474,1351-1352 */
            uint32_t j = 0;
            for (; j < NSO_KDE_RETRY; ++j) {
                philox_at(&d, ST_HT, 0, a, j, 0, w);
                double x = pow10m1(kde_sample(&t->kde[NS_KDE_HT], w));
                if (x >= 0) {                                              /* S:1351 / S:901 */
                    remainder = nso_f64_to_i64_sat(mr ? nearbyint(x) : x);
                    if (x >= 2147483648.0) ++nso_edges[NSO_EDGE_REM_HUGE];
                    if (remainder > NSO_LEN_DRAW_MAX) { remainder = NSO_LEN_DRAW_MAX; ++nso_edges[NSO_EDGE_REM_SAT]; }
                    break;
                }
            }
            if (j == NSO_KDE_RETRY) remainder = 0;
            for (j = 0; j < NSO_KDE_RETRY; ++j) {
                philox_at(&d, ST_RATIO, 0, a, j, 0, w);
                double x = kde_sample(&t->kde[NS_KDE_RATIO], w);
                if (0 <= x && x <= 1) { ratio = x; break; }
            }
            if (j == NSO_KDE_RETRY) ratio = 0.5;
        }
        philox_at(&d, ST_STRAND, 0, a, 0, 0, w);
        reversed = u32_to_p(w[0]) > t->strandness_rate;                   /* S:1312, S:1524-1525 */
        if (mr) reversed = (int)mr->reversed;                               /* S:860: one draw per pass */
        if (!ok) { ++epoch; fails = 0; continue; }

        /* ---- error lists ---- */
        uint32_t n_pieces = (kind == NS_KIND_ALIGNED) ? 2 * nseg - 1 : 1;
        if (o->n_pieces + n_pieces > o->cap_pieces) return -10;
        ns_piece *pc = o->pieces + o->n_pieces;
        uint64_t ev0 = o->n_events, evn = ev0;
        int64_t total = remainder;
        int overflow = 0, range = 0;
        for (uint32_t pi = 0; pi < n_pieces; ++pi) {
            nso_elist r;
            int is_gap = (kind == NS_KIND_UNALIGNED) || (pi & 1);
            uint32_t sid = is_gap ? NSO_GAP_SEG + (pi >> 1) : (pi >> 1);
            int64_t mlen = is_gap ? (kind == NS_KIND_UNALIGNED ? ref_len[0] : gap_len[pi >> 1]) : ref_len[pi >> 1];
            memset(&pc[pi], 0, sizeof pc[pi]);
            pc[pi].kind = (uint32_t)is_gap; pc[pi].ev_off = evn;
            if (kind == NS_KIND_PERFECT) { memset(&r, 0, sizeof r); r.l_new = r.middle_ref = mlen; }
            else if (is_gap) nso_unaligned_error_list(t, mlen, &d, sid, a, o->events + evn, o->cap_events - evn, &r);
            else nso_error_list(t, mlen, (int)prm->fastq, &d, sid, a, o->events + evn, o->cap_events - evn, &r);
            if (r.overflow) overflow = 1;
            if (kind != NS_KIND_PERFECT && r.range) range = 1;
            pc[pi].n_ev = (uint32_t)r.n_ev;
            pc[pi].ref_len = (uint32_t)(r.middle_ref < 0 ? 0 : r.middle_ref);
            /* emitted length = ref_len + ins - del over the stored events (collisions already folded in) */
            int64_t ol = (r.middle_ref < 0 ? 0 : r.middle_ref) + r.shift;
            pc[pi].out_len = (uint32_t)ol;
            evn += r.n_ev;
            if (!is_gap) total += r.l_new;                                  /* S:1362 (gaps are not counted) */
            if (kind == NS_KIND_UNALIGNED) total = r.middle_ref;            /* S:1503 */
        }
        if (range) { ++nso_range_redraws; if (!mr) { ++epoch; fails = 0; } continue; }       /* the attempt is dropped, new lengths (a limit of the 8-byte event record) */
        if (overflow) return -11;
        if (tx && kind != NS_KIND_UNALIGNED) {                              /* S:1143-1144: middle_ref > ref_trx_len -> start over */
            if ((int64_t)pc[0].ref_len > trx_len) continue;
            total = remainder + pc[0].out_len;
        } else
        if (mr) {                                                           /* S:907-946: middle_ref and gap lengths count; --perfect: S:896-897 */
            int64_t tot = remainder; int restart = 0;
            for (uint32_t pi = 0; pi < n_pieces && !restart; pi += 2) { if (tot + pc[pi].ref_len > prm->max_len) restart = 1; else tot += pc[pi].ref_len; }
            for (uint32_t pi = 1; pi < n_pieces && !restart; pi += 2) { if (tot + pc[pi].out_len > prm->max_len) restart = 1; else tot += pc[pi].out_len; }
            if (restart || tot < prm->min_len || tot > prm->max_len) continue;
            total = tot;
        } else
        if (total < prm->min_len || total > prm->max_len) {                 /* S:1367-1368 / S:1503-1504 */
            if (kind == NS_KIND_UNALIGNED) continue;
            if (++fails >= NSO_EPOCH_FAILS) { ++epoch; fails = 0; }
            continue;
        }
        /* ---- head / tail (S:1377-1382) ---- */
        int64_t head = 0, tail = 0;
        if (kind == NS_KIND_ALIGNED && remainder != 0) {
            head = (int64_t)nearbyint((double)remainder * ratio);          /* Python round(): half to even */
            tail = remainder - head;
        }
        /* ---- positions (S:1388-1389, 1510, 1557) ---- */
        int pos_ok = 1;
        int64_t seq_len = head + tail;
        nso_iv *ir_iv = NULL; int ir_n = 0, ir_polya = 0;                  /* intron retention: the genomic intervals of the read */
        for (uint32_t pi = 0; pi < n_pieces; ++pi) {
            uint32_t sid = pc[pi].kind ? NSO_GAP_SEG + (pi >> 1) : (pi >> 1);
            uint32_t chrom = 0; uint64_t pos = 0;
            if (pc[pi].kind && kind == NS_KIND_ALIGNED && gap_len[pi >> 1] == 0) {   /* S:1553-1554 */
                pc[pi].ref_len = 0; pc[pi].out_len = 0; pc[pi].n_ev = 0;
            } else if (tx && kind != NS_KIND_UNALIGNED) {
                chrom = trx_chrom;
                if (tx->ir && prm->model_ir && kind == NS_KIND_ALIGNED && pc[pi].ref_len) {      /* S:1156-1160 */
                    const ns_ir_tables *ir = tx->ir;
                    const uint32_t n_items = ir->item_off[trx_chrom + 1] - ir->item_off[trx_chrom];
                    double *u = (double *)malloc(sizeof(double) * (n_items + 1));
                    uint8_t *ret = (uint8_t *)calloc(n_items + 1, 1);
                    for (uint32_t k2 = 0; k2 < n_items; ++k2) {                /* (at most one draw per item; only the introns use theirs) */
                        philox_at(&d, ST_IR, 0, a, k2 >> 1, 0, w);
                        u[k2] = (k2 & 1) ? u53_to_p(w[2], w[3]) : u53_to_p(w[0], w[1]);
                    }
                    if (n_items && nso_ir_states(ir, trx_chrom, u, ret)) {
                        ir_iv = (nso_iv *)malloc(sizeof(nso_iv) * (n_items + 1));
                        philox_at(&d, ST_POS, sid, a, 0, 0, w);
                        ir_n = nso_extract_read_pos(ir, trx_chrom, ret, pc[pi].ref_len, trx_len, u53_to_p(w[0], w[1]),
                                                    tx->polya && tx->polya[trx_chrom], ir_iv, n_items + 1, &ir_polya);
                        if (ir_n <= 0) { free(ir_iv); ir_iv = NULL; ir_n = 0; }
                    }
                    free(u); free(ret);
                    if (ir_iv) {
                        int missing = 0;                                       /* S:1167-1169: chromosome not in the genome FASTA */
                        for (int z = 0; z < ir_n; ++z) if (ir_iv[z].chrom == NS_IR_NO_CHROM) missing = 1;
                        if (missing) { free(ir_iv); ir_iv = NULL; pos_ok = 0; break; }
                        pos = ir_iv[0].start;                                  /* S:1175 */
                    }
                }
                if (!ir_iv) {                                              /* extract_read_trx, S:1683-1691 */
                    philox_at(&d, ST_POS, sid, a, 0, 0, w);
                    uint64_t span = (uint64_t)(trx_len - (int64_t)pc[pi].ref_len) + 1;
                    pos = (uint64_t)(u53_to_p(w[0], w[1]) * (double)span);
                    if (pos >= span) pos = span - 1;
                }
            } else if (tx) {                                              /* extract_read("transcriptome", len), S:1695-1703 */
                if (extract_trx_unaligned(ref->chrom_off, ref->nchrom, pc[pi].ref_len, &d, sid, a, &chrom, &pos)) { pos_ok = 0; break; }
            } else if (mg) {                                              /* extract_read("metagenome", len, species), S:1704-1749 */
                int sp = (mr && !pc[pi].kind) ? (int)mr->species[pi >> 1] : -1;     /* gaps / unaligned reads: any species (S:1557, 1510) */
                if (nso_extract_meta(mg, ref->chrom_off, ref->circular, pc[pi].ref_len, sp, &d, sid, a, &chrom, &pos) < 0) { pos_ok = 0; break; }
            } else if (extract_pos(ref->chrom_off, ref->nchrom, ref->circular, pc[pi].ref_len, &d, sid, a, &chrom, &pos)) {
                pos_ok = 0; break;
            }
            pc[pi].chrom = chrom; pc[pi].pos = (uint32_t)pos;
            pc[pi].ref_gpos = ref->chrom_off[chrom] + pos;
            if (ir_iv) pc[pi].ref_gpos = NS_SPLICED_BASE + o->spliced_bytes + 64;      /* slot: 64 bytes of padding, the bases, padding */
            seq_len += pc[pi].out_len;
        }
        if (!pos_ok) { ++epoch; fails = 0; continue; }
        uint8_t *ir_seq = NULL;                                            /* S:1161-1178: the stretch as the genome has it */
        if (ir_iv) {
            const ns_ir_tables *ir = tx->ir;
            const int64_t rl = pc[0].ref_len;
            ir_seq = (uint8_t *)malloc((size_t)rl + 1);
            if (nso_splice(ir, ir_iv, ir_n, ir_seq, rl) != rl) { free(ir_seq); free(ir_iv); return -31; }
            for (int64_t i = 0; i < rl; ++i) ir_seq[i] = nso_normalise_base(ir_seq[i]);
            const uint64_t slot = 64 + (((uint64_t)rl + 64 + 15) & ~15ull);
            if (o->spliced) {
                if (o->spliced_bytes + slot > o->cap_spliced) { free(ir_seq); free(ir_iv); return -32; }
                memcpy(o->spliced + o->spliced_bytes + 64, ir_seq, (size_t)rl);
            }
            o->spliced_bytes += slot;
        }
        int64_t polya_len = 0;                                             /* S:1046-1053, 1206-1209, 1683-1691 */
        if (tx && kind != NS_KIND_UNALIGNED && tx->polya && tx->polya[trx_chrom] &&
            (ir_iv ? ir_polya : (int64_t)pc[0].pos + (int64_t)pc[0].ref_len + 10 >= trx_len)) {
            philox_at(&d, ST_TRX, 0, a, 1, 0, w);
            polya_len = (int64_t)fma(tx->polya_scale, -nso_log(u32_to_p(w[0])), 2.0);      /* int(expon.rvs(loc=2, scale)) */
            if (polya_len > 65535) polya_len = 65535;
            seq_len += polya_len;
        }
        uint64_t gidx = prm->first_read + index;
        /* name (S:1390-1402, 1332-1343, 1511, 1529-1534) */
        char name[4096]; int nl = 0; char num[32];
        int first = 1;
        for (uint32_t pi = 0; pi < n_pieces; ++pi) {
            if (pc[pi].kind && kind == NS_KIND_ALIGNED) {
                if (!mg) continue;                                         /* gaps are not named in genome mode */
                memcpy(name + nl, ";gap_", 5); nl += 5;                    /* S:970-971 */
                nl += u64_digits(pc[pi].out_len, name + nl);
                continue;
            }
            if (!first) name[nl++] = ';';
            first = 0;
            const char *cn = ref->names[pc[pi].chrom];
            size_t l = strlen(cn); memcpy(name + nl, cn, l); nl += (int)l;
            name[nl++] = '_'; nl += u64_digits(pc[pi].pos, name + nl);
        }
        const char *tag = kind == NS_KIND_ALIGNED ? "_aligned_" : kind == NS_KIND_PERFECT ? "_perfect_" : "_unaligned_";
        memcpy(name + nl, tag, strlen(tag)); nl += (int)strlen(tag);
        nl += u64_digits(gidx, name + nl);
        if (kind == NS_KIND_ALIGNED && nseg > 1) { memcpy(name + nl, "_chimeric", 9); nl += 9; }
        if (ir_iv) {                                                       /* S:1189-1192 */
            int any = 0;
            for (int z = 0; z < ir_n; ++z) {
                if (!ir_iv[z].retained) continue;
                if (nl > 3900) { free(ir_seq); free(ir_iv); return -33; }
                if (!any) { memcpy(name + nl, "_RetainedIntron_", 16); nl += 16; any = 1; }
                nl += u64_digits(ir_iv[z].start, name + nl); name[nl++] = '-';
                nl += u64_digits(ir_iv[z].end, name + nl); name[nl++] = ';';
            }
        }
        name[nl++] = '_'; name[nl++] = reversed ? 'R' : 'F';
        name[nl++] = '_'; nl += u64_digits((uint64_t)head, name + nl);
        name[nl++] = '_';
        first = 1;
        for (uint32_t pi = 0; pi < n_pieces; ++pi) {
            if (pc[pi].kind && kind == NS_KIND_ALIGNED) continue;
            if (!first) name[nl++] = ';';
            first = 0;
            nl += u64_digits(pc[pi].ref_len, name + nl);
        }
        name[nl++] = '_'; nl += u64_digits((uint64_t)(tail + polya_len), name + nl);      /* S:1211-1213: tail + polya_len */
        (void)num;

        /* ---- -k: homopolymer filter + mutate_homo on every aligned segment (S:1406-1414); lengths change here ---- */
        uint8_t *hp_seq[2 * NSO_MAX_SEG], *hp_q[2 * NSO_MAX_SEG];
        uint8_t *hp_log = NULL; uint64_t hp_log_len = 0, hp_log_cap = 0;
        const int hp_on = (prm->kmer_bias && kind == NS_KIND_ALIGNED);
        int hp_range = 0;
        memset(hp_seq, 0, sizeof hp_seq); memset(hp_q, 0, sizeof hp_q);
        if (hp_on) {
            for (uint32_t pi = 0; pi < n_pieces; pi += 2) {
                int64_t rl = pc[pi].ref_len;
                uint32_t sid = pi >> 1;
                uint8_t *segbuf = (uint8_t *)malloc((size_t)rl + 1);
                if (ir_seq) memcpy(segbuf, ir_seq, (size_t)rl); else fetch_segment(ref, pc[pi].chrom, pc[pi].pos, rl, segbuf);
                for (int64_t x = 0; x < rl; ++x) segbuf[x] = resolve_base(segbuf[x], &d, sid, a, (uint64_t)x);
                int64_t sh = 0;
                ns_event *pev = o->events + pc[pi].ev_off;
                pc[pi].n_ev = (uint32_t)nso_hp_filter(segbuf, rl, pev, pc[pi].n_ev, (int64_t)prm->kmer_bias, &sh);   /* S:1920-1947 */
                int64_t l1 = rl + sh;
                uint8_t *s1 = (uint8_t *)malloc((size_t)l1 + 1), *c1 = (uint8_t *)malloc((size_t)l1 + 1);
                uint64_t txt_cap = 0;
                for (uint32_t j = 0; j < pc[pi].n_ev; ++j) txt_cap += 2u * NS_EV_LEN(pev[j].info);
                nso_logrow *rows = prm->emit_errlog ? (nso_logrow *)malloc(sizeof(nso_logrow) * (pc[pi].n_ev + 1)) : NULL;
                uint8_t *txt = prm->emit_errlog ? (uint8_t *)malloc(txt_cap + 1) : NULL;
                uint64_t txt_len = 0;
                int64_t ol = nso_mutate_read(segbuf, rl, pev, pc[pi].n_ev, &d, sid, a, s1, c1, l1, rows, txt, &txt_len);
                if (ol != l1) return -21;
                if (prm->emit_errlog) {
                    for (uint32_t j = 0; j < pc[pi].n_ev; ++j) {
                        const char *tn = rows[j].type == NS_MIS ? "mis" : rows[j].type == NS_INS ? "ins" : "del";
                        uint64_t nb = (uint64_t)nl + 64 + 2u * rows[j].len;
                        if (hp_log_len + nb > hp_log_cap) { hp_log_cap = 2 * (hp_log_cap + nb) + 4096; hp_log = (uint8_t *)realloc(hp_log, hp_log_cap); }
                        uint8_t *q = hp_log + hp_log_len;
                        memcpy(q, name, (size_t)nl); q += nl;
                        q += sprintf((char *)q, "\t%u\t%s\t%u\t", rows[j].pos, tn, rows[j].len);
                        memcpy(q, txt + rows[j].ref_off, rows[j].len); q += rows[j].len; *q++ = '\t';
                        memcpy(q, txt + rows[j].new_off, rows[j].len); q += rows[j].len; *q++ = '\n';
                        hp_log_len = (uint64_t)(q - hp_log);
                    }
                }
                int64_t l2 = -1;
                uint64_t cnt0[NSO_HP_N];
                memcpy(cnt0, nso_hp, sizeof cnt0);
                for (int64_t cap2 = 2 * l1 + 4096; l2 == -1; cap2 *= 4) {                             /* (a model may grow every run many times over) */
                    free(hp_seq[pi]); free(hp_q[pi]);
                    memcpy(nso_hp, cnt0, sizeof cnt0);                                                /* (the counters see the run that counts) */
                    hp_seq[pi] = (uint8_t *)malloc((size_t)cap2);
                    hp_q[pi] = prm->fastq ? (uint8_t *)malloc((size_t)cap2) : NULL;                 /* quality CLASS of every final base */
                    l2 = nso_mutate_homo(t, s1, prm->fastq ? c1 : NULL, l1, (int64_t)prm->kmer_bias, &d, sid, a, hp_seq[pi], hp_q[pi], cap2);   /* S:1413-1414 */
                }
                free(segbuf); free(s1); free(c1); free(rows); free(txt);
                if (l2 < 0) { hp_range = 1; break; }                                                  /* the edits left the shift field of the event record */
                seq_len += l2 - (int64_t)pc[pi].out_len;
                pc[pi].out_len = (uint32_t)l2;
            }
        }
#define NSO_HP_FREE() do { for (uint32_t z_ = 0; z_ < n_pieces; ++z_) { free(hp_seq[z_]); free(hp_q[z_]); } free(hp_log); } while (0)
        if (hp_range && tx) { NSO_HP_FREE(); free(ir_seq); free(ir_iv); return -23; }   /* (a transcriptome candidate is committed by then: the call fails) */
        if (hp_range) { NSO_HP_FREE(); free(ir_seq); free(ir_iv); ++nso_range_redraws; ++epoch; fails = 0; continue; }   /* dropped like a failed final length check */
        if (!(tx && kind != NS_KIND_UNALIGNED) &&                                        /* (no length limits on aligned transcriptome reads) */
            (seq_len < prm->min_len || seq_len > prm->max_len)) { NSO_HP_FREE(); free(ir_seq); free(ir_iv); ++epoch; fails = 0; continue; }   /* S:1429-1430, S:1518-1519 */

        /* ---- accepted: materialise ---- */
        ns_read *rd = &o->reads[index];
        memset(rd, 0, sizeof *rd);
        rd->piece_off = (uint32_t)o->n_pieces; rd->n_pieces = (uint16_t)n_pieces; rd->reversed = (uint8_t)reversed;
        rd->head = (uint32_t)head; rd->tail = (uint32_t)tail; rd->seq_len = (uint32_t)seq_len; rd->attempts = a;
        rd->rec_off = o->record_bytes;

        uint64_t need = (uint64_t)nl + 2 + (uint64_t)seq_len + 1 + (prm->fastq ? (uint64_t)seq_len + 3 : 0);
        if (o->record_bytes + need > o->cap_records) return -12;
        uint8_t *rec = o->records + o->record_bytes;
        rec[0] = prm->fastq ? '@' : '>';
        memcpy(rec + 1, name, (size_t)nl); rec[1 + nl] = '\n';
        uint8_t *seq = rec + nl + 2;
        uint8_t *qual = prm->fastq ? seq + seq_len + 3 : NULL;
        int64_t wq = 0;                                      /* cursor in pre-revcomp coordinates */
        for (int64_t i = 0; i < head; ++i) {                 /* S:1426 */
            seq[wq] = ht_letter(&d, ST_HEAD, a, (uint32_t)i);
            if (qual) qual[wq] = qual_at(t, NS_Q_HT, &d, ST_HTQ, 0, a, (uint64_t)i);   /* S:1421-1423 */
            ++wq;
        }
        for (uint32_t pi = 0; pi < n_pieces; ++pi) {
            uint32_t sid = pc[pi].kind ? NSO_GAP_SEG + (pi >> 1) : (pi >> 1);
            int64_t rl = pc[pi].ref_len;
            if (hp_on && !pc[pi].kind) {
                memcpy(seq + wq, hp_seq[pi], pc[pi].out_len);
                if (qual) for (int64_t m = 0; m < (int64_t)pc[pi].out_len; ++m)                  /* one draw per FINAL position of the piece */
                    qual[wq + m] = qual_at(t, hp_q[pi][m], &d, ST_QUAL, sid, a, (uint64_t)m);
                wq += pc[pi].out_len;
                o->total_ref_bases += (uint64_t)rl;
                continue;
            }
            uint8_t *segbuf = (uint8_t *)malloc((size_t)rl + 1);
            uint8_t *cls = (uint8_t *)malloc((size_t)pc[pi].out_len + 1);
            uint64_t txt_cap = 0;
            for (uint32_t j = 0; j < pc[pi].n_ev; ++j) txt_cap += 2u * NS_EV_LEN(o->events[pc[pi].ev_off + j].info);
            int want_log = (!pc[pi].kind && prm->emit_errlog);
            nso_logrow *rows = want_log ? (nso_logrow *)malloc(sizeof(nso_logrow) * (pc[pi].n_ev + 1)) : NULL;
            uint8_t *txt = want_log ? (uint8_t *)malloc(txt_cap + 1) : NULL;
            uint64_t txt_len = 0;
            if (ir_seq) memcpy(segbuf, ir_seq, (size_t)rl); else fetch_segment(ref, pc[pi].chrom, pc[pi].pos, rl, segbuf);
            for (int64_t x = 0; x < rl; ++x) segbuf[x] = resolve_base(segbuf[x], &d, sid, a, (uint64_t)x);   /* S:1406 */
            int64_t ol = nso_mutate_read(segbuf, rl, o->events + pc[pi].ev_off, pc[pi].n_ev, &d, sid, a, seq + wq,
                                         cls, seq_len - wq - tail, rows, txt, &txt_len);
            if (ol != (int64_t)pc[pi].out_len) { free(segbuf); free(cls); free(rows); free(txt); return -13; }
            if (qual) for (int64_t m = 0; m < ol; ++m)
                qual[wq + m] = qual_at(t, pc[pi].kind ? NS_Q_UNMAPPED : cls[m], &d, ST_QUAL, sid, a, (uint64_t)m);
            if (want_log) {                                               /* S:2006-2008 */
                for (uint32_t j = 0; j < pc[pi].n_ev; ++j) {
                    const char *tn = rows[j].type == NS_MIS ? "mis" : rows[j].type == NS_INS ? "ins" : "del";
                    uint64_t nb = (uint64_t)nl + 64 + 2u * rows[j].len;
                    if (o->errlog_bytes + nb > o->cap_errlog) { free(segbuf); free(cls); free(rows); free(txt); return -14; }
                    uint8_t *p = o->errlog + o->errlog_bytes;
                    memcpy(p, name, (size_t)nl); p += nl;
                    p += sprintf((char *)p, "\t%u\t%s\t%u\t", rows[j].pos, tn, rows[j].len);
                    memcpy(p, txt + rows[j].ref_off, rows[j].len); p += rows[j].len; *p++ = '\t';
                    memcpy(p, txt + rows[j].new_off, rows[j].len); p += rows[j].len; *p++ = '\n';
                    o->errlog_bytes = (uint64_t)(p - o->errlog);
                }
            }
            wq += ol;
            o->total_ref_bases += (uint64_t)rl;
            free(segbuf); free(cls); free(rows); free(txt);
        }
        if (hp_on && hp_log_len) {
            if (o->errlog_bytes + hp_log_len > o->cap_errlog) { NSO_HP_FREE(); return -14; }
            memcpy(o->errlog + o->errlog_bytes, hp_log, hp_log_len);
            o->errlog_bytes += hp_log_len;
        }
        NSO_HP_FREE();
        for (int64_t k2 = 0; k2 < polya_len; ++k2) {          /* S:1224-1225; qualities: popped from the end of the ht draw, S:1229-1231 */
            seq[wq] = 'A';
            if (qual) qual[wq] = qual_at(t, NS_Q_HT, &d, ST_HTQ, 0, a, (uint64_t)(head + tail + polya_len - 1 - k2));
            ++wq;
        }
        if (o->polya) o->polya[index] = (uint16_t)polya_len;
        for (int64_t i = 0; i < tail; ++i) {                  /* S:1427 */
            seq[wq] = ht_letter(&d, ST_TAIL, a, (uint32_t)i);
            if (qual) qual[wq] = qual_at(t, NS_Q_HT, &d, ST_HTQ, 0, a, (uint64_t)(head + i));
            ++wq;
        }
        if (wq != seq_len) return -15;
        if (reversed) {                                       /* S:1433-1435, reverse_complement S:1675-1680 */
            for (int64_t i = 0, j = seq_len - 1; i <= j; ++i, --j) {
                uint8_t x = seq[i], y = seq[j];
                uint8_t cx = x == 'A' ? 'T' : x == 'T' ? 'A' : x == 'C' ? 'G' : x == 'G' ? 'C' : x;
                uint8_t cy = y == 'A' ? 'T' : y == 'T' ? 'A' : y == 'C' ? 'G' : y == 'G' ? 'C' : y;
                seq[i] = cy; seq[j] = cx;
                if (qual) { uint8_t tq = qual[i]; qual[i] = qual[j]; qual[j] = tq; }
            }
        }
        if (prm->uracil) for (int64_t i = 0; i < seq_len; ++i) if (seq[i] == 'T') seq[i] = 'U';      /* S:1247-1248 */
        seq[seq_len] = '\n';
        if (qual) {                                           /* S:1440-1443 */
            seq[seq_len + 1] = '+'; seq[seq_len + 2] = '\n';
            for (int64_t i = 0; i < seq_len; ++i) qual[i] = (uint8_t)(qual[i] + 33);
            qual[seq_len] = '\n';
        }
        o->record_bytes += need;
        o->n_pieces += n_pieces;
        o->n_events = evn;
        o->total_bases += (uint64_t)seq_len;
        free(ir_seq); free(ir_iv);
        return 0;
    }
    return -16;
}

/* Batch entry: same inputs as ns_generate, host buffers for every output. */
int nso_generate(const ns_model_tables *t, const uint8_t *bases, const uint64_t *chrom_off, uint32_t nchrom,
                 const uint8_t *circular, const char *names_blob, const ns_params *prm, nso_out *o) {
    const char **names = (const char **)malloc(sizeof(char *) * (nchrom + 1));
    const char *p = names_blob;
    for (uint32_t c = 0; c < nchrom; ++c) { names[c] = p; p += strlen(p) + 1; }
    nso_ref ref = {bases, chrom_off, nchrom, circular, names};
    o->n_pieces = o->n_events = o->record_bytes = o->errlog_bytes = o->total_bases = o->total_ref_bases = 0;
    int rc = 0;
    for (uint64_t i = 0; i < prm->n_reads && rc == 0; ++i) rc = gen_read(t, &ref, prm, i, o, NULL, NULL, NULL, NULL);
    free((void *)names);
    return rc;
}

/* transcriptome batch: simulation_aligned_transcriptome (S:1043-1263) / simulation_unaligned("transcriptome").
 *
 * Transcript and aligned length of the aligned reads (S:1080-1104).  The reference worker keeps ONE sample of num_simulate points of the
 * 2-D KDE (transcript length, aligned length), takes for every picked transcript the point whose first coordinate is nearest
 * (select_nearest_kde2d, S:108-111) — so inside one sample a transcript always gets the SAME aligned length — remembers the transcripts
 * it has used (trx_sampled) and draws a new sample as soon as one of them is picked again (S:1087-1092).  A transcript whose length failed
 * `ref_len_aligned < ref_trx_len` is NOT remembered: it keeps failing until some other transcript repeats.  That couples the reads of a
 * worker: restated here per BLOCK of NSO_TRX_BLOCK read indices (a "virtual worker": block b holds the reads b * W .. b * W + W - 1 of
 * the run, whatever batch or rank generates them), as a walk over the block's own pick sequence:
 *   pick j: transcript = random.choices by Philox(key read b * W, ST_TRX, idx = j, sub = 2); its aligned length under the current
 *           sample = the conditional draw nso_kde2d_cond(sub = 1 + j) of the FIRST pick of that transcript inside the sample (the nearest
 *           point of a fresh, large sample is a draw from the KDE conditioned on the transcript length);
 *   a pick of a transcript that succeeded earlier in the sample starts a new sample and is evaluated under it (S:1087-1092);
 *   a successful pick is candidate c of the block: its read is generated with the key (b * W + c mod W, attempt c / W), one try; a
 *   candidate whose error list overshoots the transcript (S:1143-1144), or that cannot be placed, is dropped; the block's reads are
 *   its first W surviving candidates, in order.
 * A batch that starts inside a block walks the block from its start (dry runs for the reads in front of the batch). */
#define NSO_TRX_BLOCK 1024u
#define NSO_TRX_MAX_PICKS (1u << 22)

/* the state of the walk: which KDE sample ("epoch") is current, and for every transcript the last sample it was looked up under and
 * whether that look-up passed S:1103-1104 */
typedef struct trx_walk {
    uint32_t *seen_epoch; uint8_t *ok_epoch;      /* per entry of the expression list */
    uint32_t *epoch_io;                           /* sample counter of the run (never reused, so the arrays need no clearing) */
    uint32_t epoch;
} trx_walk;
static void trx_walk_start(trx_walk *wk) { wk->epoch = ++*wk->epoch_io; }
/* pick of transcript e.  Returns 1 when the pick needs a look-up (first pick of e under the current sample — which is a NEW sample when e
 * passed earlier under the old one, S:1087-1092: *redraw = 1), 0 when e failed before under this sample (the same nearest point, the same
 * failure: S:1098-1104 with an unchanged sampled_2d_lengths) */
static int trx_walk_visit(trx_walk *wk, uint32_t e, int *redraw) {
    int in_epoch = wk->seen_epoch[e] == wk->epoch;
    *redraw = 0;
    if (in_epoch && wk->ok_epoch[e]) { wk->epoch = ++*wk->epoch_io; in_epoch = 0; *redraw = 1; }      /* new sample, trx_sampled = set() */
    return !in_epoch;
}
static void trx_walk_record(trx_walk *wk, uint32_t e, int good) { wk->seen_epoch[e] = wk->epoch; wk->ok_epoch[e] = (uint8_t)good; }

static int trx_block(const ns_model_tables *t, const nso_ref *ref, const ns_params *prm, const nso_trx *tx, uint64_t b, nso_out *o,
                     nso_out *dry, uint32_t *seen_epoch, uint8_t *ok_epoch, uint32_t *epoch_io) {
    const uint64_t W = NSO_TRX_BLOCK, g0 = prm->first_read, g1 = g0 + prm->n_reads;
    nso_draw db; memset(&db, 0, sizeof db); db.seed = prm->seed; db.read = b * W;
    trx_walk wk = {seen_epoch, ok_epoch, epoch_io, 0};
    trx_walk_start(&wk);
    uint32_t w[4];
    uint64_t acc = 0, c = 0;
    for (uint32_t j = 0; acc < W && b * W + acc < g1; ++j) {
        if (j >= NSO_TRX_MAX_PICKS) return -41;
        philox_at(&db, ST_TRX, 0, 0, j, 2, w);
        const uint32_t e = nso_trx_pick(tx, u53_to_p(w[0], w[1]));
        const uint32_t chrom = tx->expr_chrom[e];
        const int64_t L = (int64_t)(ref->chrom_off[chrom + 1] - ref->chrom_off[chrom]);
        int redraw;
        if (!trx_walk_visit(&wk, e, &redraw)) continue;
        const int64_t y = nso_kde2d_cond(t, (double)L, &db, 0, 1u + j);
        const int good = y > 0 && y < L;                 /* S:1103-1104 */
        trx_walk_record(&wk, e, good);
        if (!good) continue;
        if (c >= 2 * W) return -42;
        nso_tread tr; tr.key_read = b * W + c % W; tr.attempt = (uint32_t)(c / W); tr.chrom = chrom; tr.ref_len = y;
        ++c;
        const uint64_t g = b * W + acc;
        int r1;
        if (g < g0) {                                    /* a read of an earlier batch: only whether it survives matters */
            dry->n_pieces = dry->n_events = dry->record_bytes = dry->errlog_bytes = dry->total_bases = dry->spliced_bytes = 0;
            tr.seq_index = 0;
            r1 = gen_read(t, ref, prm, 0, dry, NULL, NULL, tx, &tr);
        } else {
            tr.seq_index = g - g0;
            r1 = gen_read(t, ref, prm, g - g0, o, NULL, NULL, tx, &tr);
        }
        if (r1 < 0) return r1;
        if (r1 == 0) ++acc;
    }
    return 0;
}

int nso_generate_trx(const ns_model_tables *t, const uint8_t *bases, const uint64_t *chrom_off, uint32_t nchrom,
                     const uint8_t *circular, const char *names_blob, const nso_trx *tx, const ns_params *prm, nso_out *o) {
    const char **names = (const char **)malloc(sizeof(char *) * (nchrom + 1));
    const char *p = names_blob;
    for (uint32_t c = 0; c < nchrom; ++c) { names[c] = p; p += strlen(p) + 1; }
    nso_ref ref = {bases, chrom_off, nchrom, circular, names};
    o->n_pieces = o->n_events = o->record_bytes = o->errlog_bytes = o->total_bases = o->total_ref_bases = 0;
    o->spliced_bytes = 0;
    int rc = 0;
    if (prm->kind == NS_KIND_UNALIGNED) {
        for (uint64_t i = 0; i < prm->n_reads && rc == 0; ++i) rc = gen_read(t, &ref, prm, i, o, NULL, NULL, tx, NULL);
    } else if (prm->n_reads) {
        uint64_t longest = 0;
        for (uint32_t c = 0; c < nchrom; ++c) if (chrom_off[c + 1] - chrom_off[c] > longest) longest = chrom_off[c + 1] - chrom_off[c];
        nso_out dry; memset(&dry, 0, sizeof dry);          /* scratch outputs for the dry runs in front of the batch */
        ns_read dry_read; uint16_t dry_polya;
        dry.reads = &dry_read; dry.polya = &dry_polya;
        dry.cap_pieces = 8; dry.pieces = (ns_piece *)malloc(sizeof(ns_piece) * dry.cap_pieces);
        dry.cap_events = 4 * longest + 4096; dry.events = (ns_event *)malloc(sizeof(ns_event) * dry.cap_events);
        dry.cap_records = 8 * longest + 65536; dry.records = (uint8_t *)malloc(dry.cap_records);
        dry.cap_errlog = 64 * (4 * longest + 4096) + 65536; dry.errlog = prm->emit_errlog ? (uint8_t *)malloc(dry.cap_errlog) : NULL;
        dry.spliced = NULL; dry.cap_spliced = 0;
        uint32_t *seen = (uint32_t *)calloc(tx->n_expr + 1, sizeof(uint32_t));
        uint8_t *okf = (uint8_t *)calloc(tx->n_expr + 1, 1);
        uint32_t epoch = 0;
        const uint64_t W = NSO_TRX_BLOCK;
        for (uint64_t b = prm->first_read / W; b * W < prm->first_read + prm->n_reads && rc == 0; ++b)
            rc = trx_block(t, &ref, prm, tx, b, o, &dry, seen, okf, &epoch);
        free(dry.pieces); free(dry.events); free(dry.records); free(dry.errlog); free(seen); free(okf);
    }
    free((void *)names);
    return rc;
}

/* The walk of trx_block over a TAPE of the reference's own picks (tests/golden/reference_trx_walk.json): pick j is transcript pick_e[j] of
 * length L[pick_e[j]], and pick_y[j] is the ref_len_aligned the reference looked up for it.  Where the walk needs a look-up it takes the
 * tape's value; where it says "failed before under this sample" it reports the pick whose look-up it relies on (memo_of[j]; -1
 * otherwise) so that the test can check that the reference saw the same value there.  accept[j] / redraw[j] are what the reference
 * recorded as "left the inner loop" (S:1103-1104) / "drew a new sample" (S:1087-1092).  Returns the number of samples used. */
uint32_t nso_trx_walk_tape(uint32_t n_picks, const uint32_t *pick_e, const int64_t *pick_y, uint32_t n_expr, const int64_t *L,
                           uint8_t *accept, uint8_t *redraw, int64_t *memo_of) {
    uint32_t *seen = (uint32_t *)calloc(n_expr + 1, sizeof(uint32_t));
    uint8_t *okf = (uint8_t *)calloc(n_expr + 1, 1);
    int64_t *last = (int64_t *)malloc(sizeof(int64_t) * (n_expr + 1));
    uint32_t epoch = 0;
    trx_walk wk = {seen, okf, &epoch, 0};
    trx_walk_start(&wk);
    for (uint32_t j = 0; j < n_picks; ++j) {
        const uint32_t e = pick_e[j];
        int rd;
        accept[j] = 0; memo_of[j] = -1;
        const int look = trx_walk_visit(&wk, e, &rd);
        redraw[j] = (uint8_t)rd;
        if (!look) { memo_of[j] = last[e]; continue; }
        const int good = pick_y[j] > 0 && pick_y[j] < L[e];
        trx_walk_record(&wk, e, good);
        last[e] = (int64_t)j;
        accept[j] = (uint8_t)good;
    }
    free(seen); free(okf); free(last);
    return epoch;
}

/* ------------------------------------------------------------------------------------------------
 * small exported helpers for the pinning tests
 * ---------------------------------------------------------------------------------------------- */
int64_t nso_table_value(const double *cdf, uint32_t n, double p) { return table_value(cdf, n, p); }
int nso_trans_pick(const double *row, double p) { return trans_pick(row, p); }
int64_t nso_run_length(const ns_model_tables *t, int type, double p_mix, double p_len) { return run_length(t, type, p_mix, p_len); }
double nso_kde_sample(const double *data, uint64_t n, double bw, uint32_t w0, uint32_t w1, uint32_t w2) {
    ns_kde k = {data, n, bw}; uint32_t w[4] = {w0, w1, w2, 0};
    return kde_sample(&k, w);
}
double nso_pow10m1(double x) { return pow10m1(x); }
/* the chain's table questions over n draws (tests/test_lookup_probe.py: the reference of tests/lookup_probe.hip) — the same calls
 * nso_error_list makes, with p = u32_to_p(u) */
void nso_ecdf_lookup_batch(const double *hi, const double *vhi, uint32_t nseg, double vlo0, const uint32_t *u, int64_t *out, uint64_t n) {
    for (uint64_t i = 0; i < n; ++i) out[i] = nso_ecdf_lookup(hi, vhi, nseg, vlo0, u32_to_p(u[i]));
}
/* the next match length behind prev_match: the first bin with lo <= prev_match < hi, else the last (S:1891-1893), then its column */
void nso_next_match_batch(const ns_model_tables *t, const int32_t *prev_match, const uint32_t *u, int64_t *out, uint64_t n) {
    for (uint64_t i = 0; i < n; ++i) {
        uint32_t b = 0;
        for (; b < t->mm_nbins; ++b)
            if (t->mm_bin_lo[b] <= prev_match[i] && prev_match[i] < t->mm_bin_hi[b]) break;
        if (b >= t->mm_nbins) b = t->mm_nbins - 1;
        const uint32_t o = t->mm_seg_off[b];
        out[i] = nso_ecdf_lookup(t->mm_hi + o, t->mm_vhi + o, t->mm_seg_off[b + 1] - o, t->mm_vlo0[b], u32_to_p(u[i]));
    }
}
void nso_run_length_batch(const ns_model_tables *t, const int32_t *type, const uint32_t *u_mix, const uint32_t *u_len, int64_t *out, uint64_t n) {
    for (uint64_t i = 0; i < n; ++i) out[i] = run_length(t, type[i], u32_to_p(u_mix[i]), u32_to_p(u_len[i]));
}
void nso_trans_pick_batch(const ns_model_tables *t, const int32_t *state, const uint32_t *u, int64_t *out, uint64_t n) {
    for (uint64_t i = 0; i < n; ++i) out[i] = trans_pick(t->trans[state[i]], u32_to_p(u[i]));
}
/* one scalar primitive over n inputs (tests/test_math_probe.py: the same ops as tests/math_probe.hip).  in / out: 8-byte elements,
 * read as double, or as uint64 for the draw ops (NORMINV_U: u = low 32 bits; U53: a = high, b = low 32 bits).  Returns 0, -1 for an
 * unknown op. */
enum { NSO_OP_LOG = 0, NSO_OP_EXP = 1, NSO_OP_NORMINV_U = 2, NSO_OP_POW10M1 = 3, NSO_OP_U53 = 4, NSO_OP_THR_LT = 5, NSO_OP_THR_GT = 6,
       NSO_OP_F64_I64 = 7, NSO_OP_NORMINV = 8, NSO_OP_LEN_DRAW = 9 };
int nso_eval_batch(int op, const void *in, void *out, uint64_t n) {
    const double *xd = (const double *)in; const uint64_t *xu = (const uint64_t *)in;
    double *od = (double *)out; int64_t *oi = (int64_t *)out; uint64_t *ou = (uint64_t *)out;
    switch (op) {
    case NSO_OP_LOG: for (uint64_t i = 0; i < n; ++i) od[i] = nso_log(xd[i]); break;
    case NSO_OP_EXP: for (uint64_t i = 0; i < n; ++i) od[i] = nso_exp(xd[i]); break;
    case NSO_OP_NORMINV_U: for (uint64_t i = 0; i < n; ++i) od[i] = nso_norminv(u32_to_p((uint32_t)xu[i])); break;
    case NSO_OP_POW10M1: for (uint64_t i = 0; i < n; ++i) od[i] = pow10m1(xd[i]); break;
    case NSO_OP_U53: for (uint64_t i = 0; i < n; ++i) od[i] = u53_to_p((uint32_t)(xu[i] >> 32), (uint32_t)xu[i]); break;
    case NSO_OP_THR_LT:                                   /* the integer form of p < t: #{u : u32_to_p(u) < t} */
        for (uint64_t i = 0; i < n; ++i) {
            const double t = xd[i];
            if (!(t > 0.0)) { ou[i] = 0; continue; }
            if (t >= 1.0) { ou[i] = 1ull << 32; continue; }
            const double y = ceil(t * 4294967296.0 - 0.5);
            ou[i] = y <= 0.0 ? 0ull : (uint64_t)y;
        }
        break;
    case NSO_OP_THR_GT:                                   /* the integer form of p > t: the least u with u32_to_p(u) > t */
        for (uint64_t i = 0; i < n; ++i) {
            const double t = xd[i];
            if (t < 0.0) { ou[i] = 0; continue; }
            if (t >= 1.0) { ou[i] = 1ull << 32; continue; }
            const double y = floor(t * 4294967296.0 - 0.5) + 1.0;
            ou[i] = y <= 0.0 ? 0ull : (uint64_t)y;
        }
        break;
    case NSO_OP_F64_I64: for (uint64_t i = 0; i < n; ++i) oi[i] = nso_f64_to_i64_sat(xd[i]); break;
    case NSO_OP_NORMINV: for (uint64_t i = 0; i < n; ++i) od[i] = nso_norminv(xd[i]); break;
    case NSO_OP_LEN_DRAW: for (uint64_t i = 0; i < n; ++i) oi[i] = len_draw(xd[i]); break;
    default: return -1;
    }
    return 0;
}
uint8_t nso_qual_value(const ns_model_tables *t, int cls, uint32_t h) { return qual_value(t, cls, h); }
int nso_extract_pos(const uint64_t *chrom_off, uint32_t nchrom, const uint8_t *circular, int64_t length,
                    uint64_t seed, uint64_t read, uint32_t seg, uint32_t attempt, uint32_t *chrom, uint64_t *pos) {
    nso_draw d; memset(&d, 0, sizeof d); d.seed = seed; d.read = read;
    return extract_pos(chrom_off, nchrom, circular, length, &d, seg, attempt, chrom, pos);
}
/* extract_read's position walk for a given randint value (S:1767-1780); -1 = redraw */
int nso_extract_walk(const uint64_t *chrom_off, uint32_t nchrom, uint64_t ref_pos, int64_t length, uint32_t *chrom, uint64_t *pos) {
    for (uint32_t c = 0; c < nchrom; ++c) {
        uint64_t cl = chrom_off[c + 1] - chrom_off[c];
        if (ref_pos + (uint64_t)length <= cl) { *chrom = c; *pos = ref_pos; return 0; }
        else if (ref_pos < cl) return -1;
        else ref_pos -= cl;
    }
    return -1;
}
void nso_case_convert(uint8_t *seq, int64_t n, nso_draw *d, uint32_t seg, uint32_t attempt) {
    for (int64_t x = 0; x < n; ++x) seq[x] = resolve_base(nso_normalise_base(seq[x]), d, seg, attempt, (uint64_t)x);
}

/* ------------------------------------------------------------------------------------------------
 * metagenome batch: simulation_aligned_metagenome (S:814-1040) / simulation_unaligned("metagenome") (S:1482-1549).
 * One call = one worker.  Pass p = one iteration of the reference's `while remaining_reads > 0` loop: fresh lengths for
 * all remaining reads, assign_species with the bases simulated so far, ONE strand draw, then one try per read in the
 * sorted order; accepted reads are numbered consecutively in that order (S:909-911).
 * inside a pass the reference hands the lengths of a rejected read to the next loop index; here every
 * read keeps its own entry of the sorted list and a rejected read simply waits for the next pass.
 * ---------------------------------------------------------------------------------------------- */
/* per-pass record of the last nso_generate_meta call (test infrastructure): np_spec = the reads the pass's V lengths can cover
 * (segment counts in descending order, S:781-782, at most the remaining reads), np = the reads assign_species did assign (fewer when
 * every quota is used up before the lengths are).  Passes with V == 0 are not recorded. */
#define NSO_META_PASS_LOG 4096
static uint64_t g_meta_np_spec[NSO_META_PASS_LOG], g_meta_np[NSO_META_PASS_LOG];
static uint32_t g_meta_passes;
uint32_t nso_meta_pass_log(uint64_t *np_spec, uint64_t *np, uint32_t cap) {
    const uint32_t k = g_meta_passes < cap ? g_meta_passes : cap;
    for (uint32_t i = 0; i < k; ++i) { np_spec[i] = g_meta_np_spec[i]; np[i] = g_meta_np[i]; }
    return g_meta_passes;
}

int nso_generate_meta(const ns_model_tables *t, const uint8_t *bases, const uint64_t *chrom_off, uint32_t nchrom,
                      const uint8_t *circular, const char *names_blob, const nso_meta *mg, const ns_params *prm, nso_out *o,
                      double *species_bases_out) {
    const char **names = (const char **)malloc(sizeof(char *) * (nchrom + 1));
    const char *pn = names_blob;
    for (uint32_t c = 0; c < nchrom; ++c) { names[c] = pn; pn += strlen(pn) + 1; }
    nso_ref ref = {bases, chrom_off, nchrom, circular, names};
    o->n_pieces = o->n_events = o->record_bytes = o->errlog_bytes = o->total_bases = o->total_ref_bases = 0;
    const uint64_t n = prm->n_reads;
    int rc = 0;
    g_meta_passes = 0;
    if (prm->kind == NS_KIND_UNALIGNED) {                /* random species per read, otherwise the genome-mode loop */
        for (uint64_t i = 0; i < n && rc == 0; ++i) rc = gen_read(t, &ref, prm, i, o, NULL, mg, NULL, NULL);
        free((void *)names);
        return rc;
    }
    const int perfect = prm->kind == NS_KIND_PERFECT;                    /* S:838-842, 879-910: no errors, no head/tail, quotas never updated */
    int32_t *nseg_orig = (int32_t *)malloc(sizeof(int32_t) * (n + 1));
    for (uint64_t j = 0; j < n; ++j) {                    /* num_segment, S:825-828 */
        nseg_orig[j] = 1;
        if (prm->chimeric) {
            nso_draw dj; memset(&dj, 0, sizeof dj); dj.seed = prm->seed; dj.read = prm->first_read + j;
            uint32_t w[4]; philox_at(&dj, ST_NSEG, 0, 0, 0, 0, w);
            int64_t v = table_value(t->nseg_cdf, t->nseg_n, u32_to_p(w[0]));
            nseg_orig[j] = (int32_t)(v > NSO_MAX_SEG ? NSO_MAX_SEG : v);
        }
    }
    double cur_bases[256]; memset(cur_bases, 0, sizeof cur_bases);
    nso_draw db; memset(&db, 0, sizeof db); db.seed = prm->seed; db.read = prm->first_read;     /* batch-level draws */
    uint64_t passed = 0;
    for (uint32_t p = 0; passed < n && rc == 0; ++p) {
        if (p >= NSO_MAX_ATTEMPT) { rc = -16; break; }
        const uint64_t m = n - passed;
        const int32_t *segs = nseg_orig + passed;                                     /* num_segment[passed:], S:1034 */
        uint64_t D = 0;
        for (uint64_t i = 0; i < m; ++i) D += (uint64_t)segs[i];
        double *lens = (double *)malloc(sizeof(double) * (D + 1));
        uint64_t V = 0;
        for (uint64_t j = 0; j < D; ++j) {                                            /* S:852, 857 */
            uint32_t w[4];
            const uint32_t jl = (uint32_t)j, jh = (uint32_t)(j >> 32) << 1;
            philox_at(&db, ST_REFLEN, 0, p, jl, jh, w);
            double x;
            if (!prm->use_lognormal) x = kde_sample(&t->kde[NS_KDE_ALIGNED], w);
            else if (perfect) x = nso_exp(fma(prm->sd_len, nso_norminv(u32_to_p(w[2])), nso_log(prm->median_len)));      /* S:840 */
            else {                                                                                                       /* S:854-856 */
                uint32_t w2[4];
                double tot = nso_exp(fma(prm->sd_len, nso_norminv(u32_to_p(w[2])), nso_log(prm->median_len + prm->sd_len * prm->sd_len / 2)));
                philox_at(&db, ST_REFLEN, 0, p, jl, jh | 1u, w2);
                double rem = pow10m1(kde_sample(&t->kde[NS_KDE_HT], w2));
                x = rem < 0 ? -1.0 : tot - rem;
            }
            if (x >= 2147483648.0) ++nso_edges[NSO_EDGE_LEN_HUGE];
            if (perfect ? ((double)prm->min_len <= x && x <= (double)prm->max_len) : (0 < x && x <= (double)prm->max_len)) lens[V++] = x;   /* S:841 / S:857 */
        }
        if (V == 0) { free(lens); continue; }                                          /* S:858-859 */
        uint16_t *species = (uint16_t *)malloc(sizeof(uint16_t) * (V + 1));
        double *lens_sorted = (double *)malloc(sizeof(double) * (V + 1));
        int32_t *segs_sorted = (int32_t *)malloc(sizeof(int32_t) * (m + 1));
        const uint64_t P = nso_assign_species(mg, lens, V, segs, m, cur_bases, &db, p, species, lens_sorted, segs_sorted);   /* S:866-867 */
        uint32_t w[4];
        philox_at(&db, ST_STRAND, 0, p, 0, 0, w);
        const uint32_t reversed = u32_to_p(w[0]) > t->strandness_rate;                /* S:860 */
        {                                                                                 /* the pass log: np_spec and np */
            uint64_t cv = 0, n_spec = 0, n_asg = 0;
            for (uint64_t i = 0; i < m; ++i) {
                cv += (uint64_t)segs_sorted[i];
                if (cv > V) break;
                ++n_spec;
                if (cv <= P) ++n_asg;
            }
            if (g_meta_passes < NSO_META_PASS_LOG) { g_meta_np_spec[g_meta_passes] = n_spec; g_meta_np[g_meta_passes] = n_asg; }
            ++g_meta_passes;
        }
        uint64_t seg_ptr = 0, accepted = 0;
        for (uint64_t i = 0; i < m && rc == 0; ++i) {
            const uint32_t ns = (uint32_t)segs_sorted[i];
            if (seg_ptr + ns > P) break;                                              /* S:863-865 */
            int64_t rl[NSO_MAX_SEG];
            for (uint32_t s2 = 0; s2 < ns; ++s2) rl[s2] = (int64_t)nearbyint(lens_sorted[seg_ptr + s2]);   /* S:871 */
            nso_mread mr; mr.pass = p; mr.nseg = ns; mr.pos_in_pass = (uint32_t)i; mr.reversed = reversed;
            mr.seq_index = passed + accepted; mr.ref_len = rl; mr.species = species + seg_ptr;
            const uint64_t piece0 = o->n_pieces;
            int r1 = gen_read(t, &ref, prm, i, o, &mr, mg, NULL, NULL);
            if (r1 < 0) rc = r1;
            else if (r1 == 0) {
                for (uint32_t s2 = 0; s2 < ns && !perfect; ++s2)                      /* S:1001-1002 (only in the branch with errors) */
                    cur_bases[species[seg_ptr + s2]] += (double)o->pieces[piece0 + 2 * s2].ref_len;
                ++accepted;
            }
            seg_ptr += ns;
        }
        passed += accepted;
        free(lens); free(species); free(lens_sorted); free(segs_sorted);
    }
    if (species_bases_out) for (uint32_t s2 = 0; s2 < mg->nspecies; ++s2) species_bases_out[s2] = cur_bases[s2];
    free(nseg_orig); free((void *)names);
    return rc;
}

/* ================================================================================================
 * training side (second half): the counting loop of src/besthit_to_histogram.py:hist()
 * B: = src/besthit_to_histogram.py.  PARITY: pinned against the files the reference's hist() writes for the
 * alignments of tests/golden/reference_hist.json.gz (generated by tests/golden/make_hist_golden.py, which imports the
 * module with a pysam stand-in that serves the cs strings).  Restated the way the reference does it — parse_cs builds
 * two lists, hist() walks them with Python's list[i - 1] — so that it checks the engine's one-pass walk
 * (nanosim_amd/csrc/ns_cs_hist.h) independently.
 * ============================================================================================== */
typedef struct { int64_t *hist; char *op; size_t n_hist, n_op, cap; } nso_cs_lists;
static void cs_push_hist(nso_cs_lists *l, int64_t v) { if (l->n_hist + 1 > l->cap) { l->cap = 2 * l->cap + 64; l->hist = (int64_t *)realloc(l->hist, l->cap * sizeof(int64_t)); l->op = (char *)realloc(l->op, l->cap); } l->hist[l->n_hist++] = v; }
static void cs_push_op(nso_cs_lists *l, char c) { if (l->n_op + 1 > l->cap) { l->cap = 2 * l->cap + 64; l->hist = (int64_t *)realloc(l->hist, l->cap * sizeof(int64_t)); l->op = (char *)realloc(l->op, l->cap); } l->op[l->n_op++] = c; }
static int cs_is_alpha(uint8_t c) { return (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z'); }

/* parse_cs (B:41-69): items of re.findall('(:[0-9]+|\*[a-z][a-z]|[=\+\-][A-Za-z]+)') */
static void nso_parse_cs(const uint8_t *s, uint64_t n, nso_cs_lists *l) {
    int64_t mis = 0;
    int prev_mis = 0;                                  /* prev_op == "mis" (prev_op starts as "start") */
    l->n_hist = l->n_op = 0;
    uint64_t i = 0;
    while (i < n) {
        uint8_t c = s[i];
        uint64_t j = i + 1;
        int ok = 0;
        if (c == ':') { while (j < n && s[j] >= '0' && s[j] <= '9') ++j; ok = j > i + 1; }
        else if (c == '*') { ok = i + 2 < n && s[i + 1] >= 'a' && s[i + 1] <= 'z' && s[i + 2] >= 'a' && s[i + 2] <= 'z'; j = i + 3; }
        else if (c == '+' || c == '-' || c == '=') { while (j < n && cs_is_alpha(s[j])) ++j; ok = j > i + 1; }
        if (!ok) { ++i; continue; }
        const int is_mis = c == '*';
        if (!is_mis) cs_push_op(l, (char)c);                                   /* B:49-50 */
        else if (!prev_mis) cs_push_op(l, (char)c);                            /* B:51-52 */
        prev_mis = is_mis;
        if (c == '+' || c == '-') {                                            /* B:54-58 */
            if (mis != 0) { cs_push_hist(l, mis); mis = 0; }
            cs_push_hist(l, (int64_t)(j - i - 1));
        } else if (c == ':') {                                                 /* B:59-63 */
            if (mis != 0) { cs_push_hist(l, mis); mis = 0; }
            int64_t v = 0;
            for (uint64_t k = i + 1; k < j; ++k) { v = v * 10 + (s[k] - '0'); if (v > 0xffffffffll) v = 0xffffffffll; }
            cs_push_hist(l, v);
        } else if (is_mis) mis += 1;                                           /* B:64-65 ("skip" items add nothing) */
        i = j;
    }
    if (mis != 0) cs_push_hist(l, mis);                                        /* B:67-68 */
}
int nso_parse_cs_lists(const uint8_t *s, uint64_t n, int64_t *hist, char *op, uint32_t cap, uint32_t *n_hist, uint32_t *n_op) {
    nso_cs_lists l; memset(&l, 0, sizeof l);
    nso_parse_cs(s, n, &l);
    *n_hist = (uint32_t)l.n_hist; *n_op = (uint32_t)l.n_op;
    int rc = (l.n_hist > cap || l.n_op > cap) ? -1 : 0;
    if (!rc) { memcpy(hist, l.hist, l.n_hist * sizeof(int64_t)); memcpy(op, l.op, l.n_op); }
    free(l.hist); free(l.op);
    return rc;
}

static int cs_word(char op) { return op == ':' ? 0 : op == '*' ? 1 : op == '+' ? 2 : op == '-' ? 3 : 4; }   /* conv_op_to_word: match mis ins del skip */

/* hist(), the bam branch (B:316-365).  dic: [5][1001] = dic_match, dic_first_match, dic_mis, dic_ins, dic_del (add_dict, B:14-22);
 * match_list: dense cap2 x cap2 (add_match, B:25-38); error_list: rows mis, ins, del, mis0, ins0, del0 x columns mis, ins, del.
 * Returns 0; -2: list_hist shorter than list_op (an `=` item: the reference raises IndexError or counts garbage). */
int nso_cs_hist(const uint8_t *cs, const uint64_t *off, uint32_t n_aln, uint32_t cap2, uint64_t *dic, uint64_t *match_list,
                uint64_t *error_list, uint64_t *first_error, uint64_t *max_match, uint64_t *overflow) {
    nso_cs_lists l; memset(&l, 0, sizeof l);
    int64_t prev_match = 0;                            /* (the reference leaves it unbound in front of the first alignment) */
    int prev_error = 1, rc = 0;
    *max_match = 0; *overflow = 0;
#define NSO_ADD_DICT(w, v) do { int64_t v_ = (v); if (v_ <= 1000) dic[(w) * 1001 + v_] += 1; } while (0)                 /* B:14-22 */
#define NSO_ADD_MATCH(p, q) do { int64_t p_ = (p), q_ = (q), m_ = p_ > q_ ? p_ : q_; if ((uint64_t)m_ > *max_match) *max_match = (uint64_t)m_; \
        if (match_list && m_ < (int64_t)cap2) match_list[(uint64_t)p_ * cap2 + (uint64_t)q_] += 1; else *overflow += 1; } while (0)
    for (uint32_t a = 0; a < n_aln && !rc; ++a) {
        nso_parse_cs(cs + off[a], off[a + 1] - off[a], &l);                    /* B:325 */
        int flag = 1;                                                          /* B:327 */
        for (size_t i = 0; i < l.n_op; ++i) {
            const int curr = cs_word(l.op[i]);                                 /* B:329 */
            if (curr == 4) continue;                                           /* B:330 */
            if (i >= l.n_hist) { rc = -2; break; }
            if (curr != 0) {                                                   /* B:331-352 */
                const int exact_prev = cs_word(l.op[(i + l.n_op - 1) % l.n_op]);   /* list_op_unique[i - 1]: Python wraps for i = 0 */
                int pe = prev_error;
                if (exact_prev != 0) pe += 3;                                  /* prev_error += "0" */
                if (flag) { flag = 0; first_error[curr - 1] += 1; }
                else error_list[(pe - 1) * 3 + (curr - 1)] += 1;
                prev_error = curr;
                if (curr == 1) {
                    NSO_ADD_DICT(2, l.hist[i]);
                    if (exact_prev != 0) { NSO_ADD_DICT(0, 0); NSO_ADD_MATCH(prev_match, 0); prev_match = 0; }
                } else if (curr == 3) NSO_ADD_DICT(4, l.hist[i]);
                else NSO_ADD_DICT(3, l.hist[i]);
            } else {                                                           /* B:353-364 */
                const int64_t match = l.hist[i];
                if (flag) { NSO_ADD_DICT(1, match); prev_match = match; }
                else if (i == l.n_op - 1) NSO_ADD_MATCH(prev_match, match);
                else { NSO_ADD_DICT(0, match); NSO_ADD_MATCH(prev_match, match); prev_match = match; }
            }
        }
    }
#undef NSO_ADD_DICT
#undef NSO_ADD_MATCH
    free(l.hist); free(l.op);
    return rc;
}

/* hist(), the MAF branch (B:188-315): the two aligned lines of every alignment of <prefix>_besthit.maf, column by column.
 * ref / qry: the two lines of all alignments back to back (same offsets: the lines of an alignment have the same length).
 * Same counters as nso_cs_hist.  The state of the reference's loop is kept as it is — four pending run counters of which the
 * `elif` chains flush ONE per column, prev_match and prev_error reset per alignment (B:191-193), whatever is still pending
 * behind the last column is dropped, only a final match reaches match_list (B:233-234).
 * PARITY: pinned against the files the REAL hist(prefix, "maf") wrote (tests/golden/reference_hist_maf.json.gz,
 * make_hist_golden.py --maf). */
static uint8_t maf_upper(uint8_t c) { return (c >= 'a' && c <= 'z') ? (uint8_t)(c - 32) : c; }          /* str.upper(), B:195, 198 */
int nso_maf_hist(const uint8_t *ref, const uint8_t *qry, const uint64_t *off, uint32_t n_aln, uint32_t cap2, uint64_t *dic, uint64_t *match_list,
                 uint64_t *error_list, uint64_t *first_error, uint64_t *max_match, uint64_t *overflow) {
    *max_match = 0; *overflow = 0;
#define MAF_ADD_DICT(w, v) do { int64_t v_ = (v); if (v_ <= 1000) dic[(w) * 1001 + v_] += 1; } while (0)                 /* B:14-22 */
#define MAF_ADD_MATCH(p, q) do { int64_t p_ = (p), q_ = (q), m_ = p_ > q_ ? p_ : q_; if ((uint64_t)m_ > *max_match) *max_match = (uint64_t)m_; \
        if (match_list && m_ < (int64_t)cap2) match_list[(uint64_t)p_ * cap2 + (uint64_t)q_] += 1; else *overflow += 1; } while (0)
    /* the bookkeeping every flushed error run shares (B:205-213 and its eleven copies): curr = 1 mis, 2 ins, 3 del; next_state = the
     * prev_error it leaves (1..3, or 4..6 for mis0 / ins0 / del0) */
#define MAF_TRANSITION(curr, next_state) do { if (flag) { flag = 0; first_error[(curr) - 1] += 1; } \
        else { error_list[(prev_error - 1) * 3 + ((curr) - 1)] += 1; } \
        prev_error = (next_state); } while (0)
    /* a match run ends in front of an error column (B:236-244 and its two copies) */
#define MAF_FLUSH_MATCH() do { if (flag) { MAF_ADD_DICT(1, match); prev_match = match; } \
        else { MAF_ADD_DICT(0, match); MAF_ADD_MATCH(prev_match, match); prev_match = match; } match = 0; } while (0)
    for (uint32_t a = 0; a < n_aln; ++a) {
        const uint8_t *r = ref + off[a], *q = qry + off[a];
        const uint64_t n = off[a + 1] - off[a];
        int64_t prev_match = 0, match = 0, mismatch = 0, ins = 0, dele = 0;     /* B:191, 199-202 */
        int prev_error = 0, flag = 1;                                          /* B:192-193 */
        for (uint64_t i = 0; i < n; ++i) {
            const uint8_t rc = maf_upper(r[i]), qc = maf_upper(q[i]);
            if (rc == qc) {                                                    /* B:204-234 */
                if (mismatch != 0) { MAF_ADD_DICT(2, mismatch); mismatch = 0; MAF_TRANSITION(1, 1); }
                else if (ins != 0) { MAF_ADD_DICT(3, ins); ins = 0; MAF_TRANSITION(2, 2); }
                else if (dele != 0) { MAF_ADD_DICT(4, dele); dele = 0; MAF_TRANSITION(3, 3); }
                match += 1;
                if (i == n - 1 && match != 0) MAF_ADD_MATCH(prev_match, match);
            } else if (rc == '-') {                                            /* B:235-257: an inserted base */
                if (match != 0) MAF_FLUSH_MATCH();
                else if (mismatch != 0) {
                    MAF_ADD_DICT(2, mismatch); dic[0] += 1; MAF_ADD_MATCH(prev_match, 0); prev_match = 0; mismatch = 0;
                    MAF_TRANSITION(1, 4);
                }
                ins += 1;
            } else if (qc == '-') {                                            /* B:258-280: a deleted base */
                if (match != 0) MAF_FLUSH_MATCH();
                else if (mismatch != 0) {
                    MAF_ADD_DICT(2, mismatch); dic[0] += 1; MAF_ADD_MATCH(prev_match, 0); prev_match = 0; mismatch = 0;
                    MAF_TRANSITION(1, 4);
                }
                dele += 1;
            } else {                                                           /* B:281-315: a mismatch */
                if (match != 0) MAF_FLUSH_MATCH();
                else if (ins != 0) {
                    MAF_ADD_DICT(3, ins); MAF_ADD_DICT(0, match); MAF_ADD_MATCH(prev_match, 0); prev_match = 0; ins = 0;
                    MAF_TRANSITION(2, 5);
                } else if (dele != 0) {
                    MAF_ADD_DICT(4, dele); MAF_ADD_DICT(0, match); MAF_ADD_MATCH(prev_match, 0); prev_match = 0; dele = 0;
                    MAF_TRANSITION(3, 6);
                }
                mismatch += 1;
            }
        }
    }
#undef MAF_ADD_DICT
#undef MAF_ADD_MATCH
#undef MAF_TRANSITION
#undef MAF_FLUSH_MATCH
    return 0;
}
