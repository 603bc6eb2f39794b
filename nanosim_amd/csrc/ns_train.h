// ns_train.h — training side, the device kernels: the counting loops of the characterisation stage (k_cs_len, k_cs_hist),
// of the base-quality model (k_qual_mark, k_qual_count) and of the homopolymer-length model (k_hp_count, k_hp_records), and the line pairs
// of SAM records (k_sam_scan, k_sam_lines), the fit of the error-length mixtures (k_mixfit), and the lengths behind the read-length
// models (k_len_scan, k_len_flag, k_len_reduce), the split-alignment choice of chimeric reads (k_chim_scan, k_chim_select), the EM of
// the abundance quantification (k_em_estep, k_em_accum, k_em_stop), the Markov counts of the intron-retention model (k_ir_walk), and the
// best hit per read of a MAF file (k_maf_*), the SAM text of BAM records (k_bam_*), and the MD and cs text of alignments from the
// reference genome (k_calmd_*), and the index of a SAM text (k_sam_sep_count, k_sam_sep_write, k_sam_tags, k_sam_rows).  The
// walks they run are ns_cs_hist.h, ns_qual_hist.h, ns_hp_hist.h, ns_sam_pairs.h, ns_mixfit.h, ns_read_len.h, ns_chimeric.h, ns_em.h,
// ns_ir_train.h, ns_maf_best.h, ns_bam.h, ns_calmd.h and ns_sam_index.h, which also compile for the host; the host side of the calls
// (ns_cs_histograms / ns_maf_histograms, ns_qual_histograms, ns_hp_histograms / ns_hp_histograms_sam, ns_sam_pairs_build, ns_mixture_fit,
// ns_read_lengths, ns_cigar_spans / ns_chimeric_select, ns_em_quantify, ns_ir_train, ns_maf_besthit, ns_bam_to_sam, ns_calmd, ns_sam_index) is ns_train_calls.h.  Nothing here uses GenArgs or the simulation.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ns_device.h"
#include "ns_cs_hist.h"
#include "ns_qual_hist.h"
#include "ns_hp_hist.h"
#include "ns_sam_pairs.h"
#include "ns_mixfit.h"
#include "ns_read_len.h"
#include "ns_chimeric.h"
#include "ns_em.h"
#include "ns_ir_train.h"
#include "ns_maf_best.h"
#include "ns_bam.h"
#include "ns_calmd.h"
#include "ns_sam_index.h"

// ---------------------------------------------------------------------------------------------------------
// k_cs_hist: the counting loop of the characterisation stage (ns_cs_hist.h; src/besthit_to_histogram.py:316-365), one alignment per
// thread.  The 1-D histograms and the transition counters are privatised per workgroup in LDS (their hot bins — one-base mismatches,
// short matches — would serialise millions of atomics on a few addresses) and flushed once; the (previous match, next match) matrix is
// large and sparse: global atomics.
// ---------------------------------------------------------------------------------------------------------
struct CsHistDev {
    unsigned long long *dic;          // [5][1001]
    unsigned long long *err;          // [18] error_list, [3] first_error behind it
    unsigned long long *misc;         // [0] max_match [1] match_list overflow [2] `=` items
    unsigned long long *m2; uint32_t cap2;
};
#define NS_CSH_LDS_WORDS (5u * 1001u + 24u + 1u)
struct CsAccDev {
    uint32_t *l;                      // the workgroup's LDS counters: dic[5][1001], err[18], first[3], (3 spare), the largest match
    const CsHistDev *H;
    uint32_t mx;                      // largest length this thread handed to add_match
    __device__ __forceinline__ void d1(uint32_t which, uint32_t v) { if (v <= NS_CS_DICT_MAX) atomicAdd(&l[which * 1001u + v], 1u); }
    __device__ __forceinline__ void m2(uint32_t p, uint32_t s) {
        const uint32_t m = p > s ? p : s;
        mx = mx > m ? mx : m;
        if (H->m2 && m < H->cap2) atomicAdd(&H->m2[(uint64_t)p * H->cap2 + s], 1ull);
        else atomicAdd(&H->misc[1], 1ull);
    }
    __device__ __forceinline__ void err(uint32_t i) { atomicAdd(&l[5u * 1001u + i], 1u); }
    __device__ __forceinline__ void first(uint32_t i) { atomicAdd(&l[5u * 1001u + 18u + i], 1u); }
    __device__ __forceinline__ void skip() { atomicAdd(&H->misc[2], 1ull); }
};
__global__ void __launch_bounds__(256) k_cs_len(const uint64_t *__restrict__ off, uint32_t n_aln, uint32_t *__restrict__ key, uint32_t *__restrict__ idx) {
    const uint32_t a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n_aln) return;
    const uint64_t n = off[a + 1] - off[a];
    key[a] = n > 0xffffffffull ? 0xffffffffu : (uint32_t)n; idx[a] = a;
}
// qry != nullptr: the MAF branch — cs holds the reference lines, qry the query lines (maf_hist_alignment)
__global__ void __launch_bounds__(256) k_cs_hist(const uint8_t *__restrict__ cs, const uint64_t *__restrict__ off, uint32_t n_aln, CsHistDev H,
                                                 const uint32_t *__restrict__ order, const uint8_t *__restrict__ qry) {
    __shared__ uint32_t cnt[NS_CSH_LDS_WORDS];
    for (uint32_t i = threadIdx.x; i < NS_CSH_LDS_WORDS; i += blockDim.x) cnt[i] = 0;
    __syncthreads();
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid < n_aln) {
        const uint64_t a = order ? order[tid] : tid;          // visited by descending length: the 64 walks of a wavefront have similar trip counts
        const uint8_t *s = cs + off[a];
        const uint64_t n = off[a + 1] - off[a];
        // prev_match is only read before this alignment assigns it when its first op is an error: then it is what the alignments in
        // front of it left (the reference never resets it between alignments)
        CsAccDev acc{cnt, &H, 0u};
        if (qry) maf_hist_alignment(s, qry + off[a], n, acc);
        else {
            uint32_t pm = 0;
            CsBytes sb(s);                                   // (an 8-byte register window over the thread's string: ns_cs_hist.h)
            { CsCursor c; cs_cursor_init(c); int t; uint32_t l; if (cs_next_op(sb, n, c, t, l) && t != CS_MATCH) pm = cs_carry_in(cs, off, a); }
            cs_hist_alignment(sb, n, pm, nullptr, acc);
        }
        if (acc.mx) atomicMax(&cnt[NS_CSH_LDS_WORDS - 1u], acc.mx);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < NS_CSH_LDS_WORDS; i += blockDim.x) {
        const uint32_t v = cnt[i];
        if (!v) continue;
        if (i < 5u * 1001u) atomicAdd(&H.dic[i], (unsigned long long)v);
        else if (i < NS_CSH_LDS_WORDS - 1u) atomicAdd(&H.err[i - 5u * 1001u], (unsigned long long)v);
        else atomicMax(&H.misc[0], (unsigned long long)v);          // one atomic per workgroup for the largest match
    }
}

// ---------------------------------------------------------------------------------------------------------
// k_qual_mark, k_qual_count: the base-quality histograms of the training side (ns_qual_hist.h; src/model_base_qualities.py:23-79).
// MARK, one alignment per thread: the cs walk records a 2-bit mark per mismatched / inserted base (16 bases per word of `marks`, zeroed
// by the caller).  A thread meets its bases in ascending order, so it gathers a word's marks in a register and writes the word once:
// with a plain store when the word lies inside its own quality string, with an atomic OR for the string's first and last word, which
// a neighbouring alignment may share.
// COUNT streams the quality bytes and the marks once: a thread takes 16 bytes + one mark word per load, four loads in flight, wherever
// the alignments begin; the alignment of a position comes from a binary search of the offsets, then from a walk forward.  Counters:
// 32 copies of the 5 x 94 (+ 1) table per workgroup in LDS, copy = lane mod 32 = the LDS bank — `match` at the modal quality takes
// most bases, and one counter per workgroup would serialise every wavefront's 64 adds on it; a copy per bank leaves two lanes of a
// wavefront (one per 32-lane half) and the four wavefronts on an address.  A workgroup counts a contiguous span of at most 2^31 bytes
// (the caller's grid), so no 32-bit counter can wrap; the copies are summed and flushed once with 64-bit atomics.
// ---------------------------------------------------------------------------------------------------------
#define NS_QH_BINS (QH_CLASSES * NS_QUAL_VALUES + 1u)      // the last one: bytes that are no quality value
#define NS_QH_COPIES 32u
#define NS_QH_LOADS 4u
#define NS_QH_SUBTILE 4096u                                // 256 threads x 16 bytes
#define NS_QH_TILE (NS_QH_LOADS * NS_QH_SUBTILE)
#define NS_QH_OUT_SHORT (QH_CLASSES * 128u)                // the device image of ns_qual_hist: hist[5][128], n_short, n_bad_qual
#define NS_QH_OUT_BAD (QH_CLASSES * 128u + 1u)
#define NS_QH_OUT_WORDS (QH_CLASSES * 128u + 2u)
struct QualMarkDev {
    uint32_t *marks;
    uint64_t base;                    // where the aligned part begins in the quality bytes
    uint64_t w_first, w_last;         // the words a neighbouring alignment may write too
    uint64_t cur; uint32_t bits;
    __device__ __forceinline__ void flush() {
        if (!bits) return;
        if (cur == w_first || cur == w_last) atomicOr(&marks[cur], bits); else marks[cur] = bits;
    }
    __device__ __forceinline__ void mark(uint64_t i, uint32_t m) {
        const uint64_t pos = base + i, w = pos >> 4;
        if (w != cur) { flush(); cur = w; bits = 0; }
        bits |= m << (2u * (uint32_t)(pos & 15u));
    }
};
__global__ void __launch_bounds__(256) k_qual_mark(const uint8_t *__restrict__ cs, const uint64_t *__restrict__ cs_off, const uint64_t *__restrict__ qual_off,
                                                   const ns_qual_aln *__restrict__ aln, uint32_t n_aln, const uint32_t *__restrict__ order,
                                                   uint32_t *__restrict__ marks, unsigned long long *__restrict__ out) {
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= n_aln) return;
    const uint64_t a = order ? order[tid] : tid;              // by descending length of the cs strings, as k_cs_hist
    const ns_qual_aln A = aln[a];
    const uint64_t lo = qual_off[a], hi = qual_off[a + 1];
    const uint64_t aligned = hi - lo - A.head - A.tail;
    if (A.unmapped || !aligned) return;
    QualMarkDev sink{marks, lo + A.head, lo >> 4, (hi - 1u) >> 4, ~0ull, 0u};
    CsBytes sb(cs + cs_off[a]);
    const bool covered = qual_mark_alignment(sb, cs_off[a + 1] - cs_off[a], aligned, sink);
    sink.flush();
    if (!covered) atomicAdd(&out[NS_QH_OUT_SHORT], 1ull);
}
__global__ void __launch_bounds__(256) k_qual_count(const uint8_t *__restrict__ qual, const uint32_t *__restrict__ marks, const uint64_t *__restrict__ off,
                                                    const ns_qual_aln *__restrict__ aln, uint32_t n_aln, uint64_t tiles_per_wg, uint64_t n_tiles,
                                                    unsigned long long *__restrict__ out) {
    __shared__ uint32_t cnt[NS_QH_BINS * NS_QH_COPIES];
    for (uint32_t i = threadIdx.x; i < NS_QH_BINS * NS_QH_COPIES; i += blockDim.x) cnt[i] = 0;
    __syncthreads();
    uint32_t *mine = cnt + (threadIdx.x & (NS_QH_COPIES - 1u));
    const uint64_t begin = off[0], end = off[n_aln];
    const uint64_t t0 = (uint64_t)blockIdx.x * tiles_per_wg, t1 = t0 + tiles_per_wg < n_tiles ? t0 + tiles_per_wg : n_tiles;
    uint32_t a = 0, next = 0;                                 // the alignment of the last byte looked at; where the search for the next goes on
    uint64_t lo = 0, hi = 0;                                  // its bytes (hi = 0: none yet)
    ns_qual_aln A{0u, 0u, 0u, 0u};
    for (uint64_t t = t0; t < t1; ++t) {
        const uint64_t p0 = t * NS_QH_TILE + (uint64_t)threadIdx.x * 16u;
        uint4 v[NS_QH_LOADS]; uint32_t m[NS_QH_LOADS];
#pragma unroll
        for (uint32_t j = 0; j < NS_QH_LOADS; ++j) {
            const uint64_t p = p0 + (uint64_t)j * NS_QH_SUBTILE;
            v[j] = make_uint4(0u, 0u, 0u, 0u); m[j] = 0u;
            if (p < end) { v[j] = *reinterpret_cast<const uint4 *>(qual + p); m[j] = marks[p >> 4]; }     // (both buffers are padded to whole words)
        }
#pragma unroll
        for (uint32_t j = 0; j < NS_QH_LOADS; ++j) {
            const uint64_t p = p0 + (uint64_t)j * NS_QH_SUBTILE;
            const uint32_t w[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
#pragma unroll
            for (uint32_t k = 0; k < 16u; ++k) {
                const uint64_t pos = p + k;
                if (pos < begin || pos >= end) continue;
                if (pos >= hi) {                              // the next alignment that holds a byte: a few steps forward, else a search
                    for (uint32_t s = 0; s < 4u && off[next + 1u] <= pos; ++s) ++next;
                    if (off[next + 1u] <= pos) next = qual_locate(off, next + 1u, n_aln, pos);
                    a = next; next = a + 1u;
                    lo = off[a]; hi = off[a + 1u]; A = aln[a];
                }
                const uint32_t q = ((w[k >> 2] >> (8u * (k & 3u))) & 0xffu) - NS_QUAL_FIRST;
                const uint32_t bin = q < NS_QUAL_VALUES ? qual_class(pos - lo, hi - lo, A.head, A.tail, A.unmapped, (m[j] >> (2u * k)) & 3u) * NS_QUAL_VALUES + q
                                                        : NS_QH_BINS - 1u;
                atomicAdd(&mine[bin * NS_QH_COPIES], 1u);
            }
        }
    }
    __syncthreads();
    for (uint32_t bin = threadIdx.x; bin < NS_QH_BINS; bin += blockDim.x) {
        unsigned long long sum = 0;
        for (uint32_t c = 0; c < NS_QH_COPIES; ++c) sum += cnt[bin * NS_QH_COPIES + ((c + bin) & (NS_QH_COPIES - 1u))];   // (rotated: the lanes read 32 banks)
        if (sum) atomicAdd(&out[bin < NS_QH_BINS - 1u ? (bin / NS_QUAL_VALUES) * 128u + bin % NS_QUAL_VALUES : NS_QH_OUT_BAD], sum);
    }
}

// ---------------------------------------------------------------------------------------------------------
// k_hp_count, k_hp_records: the homopolymer-length model of the training side (ns_hp_hist.h; src/model_homopolymer_lengths.py:9-119 —
// not the -k stage of the simulation above).  One alignment per thread, both lines through 8-byte CsBytes windows, visited by
// descending length as k_cs_hist.  The [2][ref_len][read_len] counts: the corner below NS_HPT_CORNER in both lengths — where almost
// every homopolymer falls — is privatised per workgroup in LDS and flushed once; 2 x 48 x 48 x 4 B = 18 KB leaves eight workgroups
// (32 wavefronts, the limit) on a compute unit's 160 KB.  What lies outside goes to the caller's dense table by global atomics, or,
// beyond its caps, to the overflow counter.  A workgroup counts 256 alignments of fewer than 2^24 columns each (the host checks), so
// no 32-bit counter can wrap.  The column counters, the number of homopolymers and the overflow are summed over the wavefront first.
// k_hp_records repeats the walk and writes the homopolymers of alignment a from slot[a] on (the exclusive scan of k_hp_count's
// per-alignment numbers; slot[n_aln] is their total): nothing when the caller's buffer is too small for all of them.
// ---------------------------------------------------------------------------------------------------------
#define NS_HPT_CORNER 48u
#define NS_HPT_LDS_WORDS (2u * NS_HPT_CORNER * NS_HPT_CORNER)
enum { HPT_COLUMNS = 0, HPT_N_HP = 4, HPT_OVERFLOW = 5, HPT_MAX_REF = 6, HPT_MAX_READ = 7, HPT_WORDS = 8 };   // the device image of the small results
struct HpTrainDev {
    unsigned long long *table;        // [2][cap_ref][cap_read]
    unsigned long long *small;        // [HPT_WORDS]
    uint32_t cap_ref, cap_read;
};
struct HpTrainAcc {
    uint32_t *l;                      // the workgroup's corner of the table
    const HpTrainDev *H;
    uint32_t mx_ref, mx_read, over, col[4];
    __device__ __forceinline__ void hp(uint32_t cls, uint8_t, uint32_t ref_len, uint32_t read_len, uint32_t, uint32_t) {
        mx_ref = mx_ref > ref_len ? mx_ref : ref_len;
        mx_read = mx_read > read_len ? mx_read : read_len;
        if (ref_len >= H->cap_ref || read_len >= H->cap_read) ++over;
        else if (ref_len < NS_HPT_CORNER && read_len < NS_HPT_CORNER) atomicAdd(&l[(cls * NS_HPT_CORNER + ref_len) * NS_HPT_CORNER + read_len], 1u);
        else atomicAdd(&H->table[((uint64_t)cls * H->cap_ref + ref_len) * H->cap_read + read_len], 1ull);
    }
    __device__ __forceinline__ void columns(uint32_t ins, uint32_t del, uint32_t mis, uint32_t match) {
        col[HPC_INS] = ins; col[HPC_DEL] = del; col[HPC_MIS] = mis; col[HPC_MATCH] = match;
    }
};
__global__ void __launch_bounds__(256) k_hp_count(const uint8_t *__restrict__ ref, const uint8_t *__restrict__ qry, const uint64_t *__restrict__ off,
                                                  uint32_t n_aln, uint32_t min_hp_len, HpTrainDev H, const uint32_t *__restrict__ order,
                                                  unsigned long long *__restrict__ n_per_aln) {
    __shared__ uint32_t cnt[NS_HPT_LDS_WORDS];
    for (uint32_t i = threadIdx.x; i < NS_HPT_LDS_WORDS; i += blockDim.x) cnt[i] = 0;
    __syncthreads();
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    HpTrainAcc acc{cnt, &H, 0u, 0u, 0u, {0u, 0u, 0u, 0u}};
    uint32_t n_hp = 0;
    if (tid < n_aln) {
        const uint64_t a = order ? order[tid] : tid;
        CsBytes rb(ref + off[a]), qb(qry + off[a]);
        n_hp = hp_hist_alignment(rb, qb, off[a + 1] - off[a], min_hp_len, acc);
        n_per_aln[a] = n_hp;
    }
    // (every lane of the workgroup comes here: the wavefront sums need them all)
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t sums[6] = {acc.col[0], acc.col[1], acc.col[2], acc.col[3], n_hp, acc.over};
#pragma unroll
    for (uint32_t j = 0; j < 6u; ++j) {
        const unsigned long long s = wave_sum(sums[j]);
        if (lane == 0 && s) atomicAdd(&H.small[j], s);          // HPT_COLUMNS .. HPT_OVERFLOW
    }
    uint32_t mr = acc.mx_ref, mq = acc.mx_read;
    for (int o = 32; o > 0; o >>= 1) { mr = max(mr, (uint32_t)__shfl_xor((int)mr, o)); mq = max(mq, (uint32_t)__shfl_xor((int)mq, o)); }
    if (lane == 0 && mr) atomicMax(&H.small[HPT_MAX_REF], (unsigned long long)mr);
    if (lane == 0 && mq) atomicMax(&H.small[HPT_MAX_READ], (unsigned long long)mq);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < NS_HPT_LDS_WORDS; i += blockDim.x) {
        const uint32_t v = cnt[i];
        if (!v) continue;                                           // (an entry counted here lies inside the caps: HpTrainAcc::hp)
        const uint32_t cls = i / (NS_HPT_CORNER * NS_HPT_CORNER), r = i / NS_HPT_CORNER % NS_HPT_CORNER, q = i % NS_HPT_CORNER;
        atomicAdd(&H.table[((uint64_t)cls * H.cap_ref + r) * H.cap_read + q], (unsigned long long)v);
    }
}
struct HpRecordSink {
    ns_hp_record *rec; uint64_t at, end; uint32_t aln;
    __device__ __forceinline__ void hp(uint32_t, uint8_t base, uint32_t ref_len, uint32_t read_len, uint32_t start, uint32_t) {
        const uint32_t code = base == 'A' ? 0u : base == 'C' ? 1u : base == 'G' ? 2u : 3u;
        if (at < end) rec[at] = ns_hp_record{aln, start, ref_len, read_len << 2 | code};
        ++at;
    }
    __device__ __forceinline__ void columns(uint32_t, uint32_t, uint32_t, uint32_t) {}
};
__global__ void __launch_bounds__(256) k_hp_records(const uint8_t *__restrict__ ref, const uint8_t *__restrict__ qry, const uint64_t *__restrict__ off,
                                                    uint32_t n_aln, uint32_t min_hp_len, const uint32_t *__restrict__ order,
                                                    const unsigned long long *__restrict__ slot, ns_hp_record *__restrict__ rec, uint64_t cap_records) {
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= n_aln || slot[n_aln] > cap_records) return;
    const uint64_t a = order ? order[tid] : tid;
    if (slot[a + 1] == slot[a]) return;
    HpRecordSink sink{rec, slot[a], slot[a + 1], (uint32_t)a};
    CsBytes rb(ref + off[a]), qb(qry + off[a]);
    hp_hist_alignment(rb, qb, off[a + 1] - off[a], min_hp_len, sink);
}

// ---------------------------------------------------------------------------------------------------------
// k_sam_scan, k_sam_lines: the two aligned lines of every SAM record from CIGAR, MD and SEQ (ns_sam_pairs.h; src/pairwise2maf.py:38-82
// behind sam2pairwise).  SCAN, one record per thread: CIGAR and MD through 8-byte CsBytes windows as k_cs_hist reads its strings; it
// writes the record's figures, its number of columns (0 for a bad record: the exclusive scan of these is aln_off) and its exceptions.
// LINES is the byte mover and is driven by the OUTPUT: a thread owns one aligned 16-byte word of each line, a wavefront 1 KiB of
// consecutive bytes, wherever the records begin — so a wavefront is as busy on ten-column records as on one of 8 kb, and a word has
// exactly one writer: the records whose bytes share it are all composed by that thread and leave in one 16-byte store per line (the
// buffers are padded to whole words; nothing is read back, merged or stored bytewise).  The first record of a wavefront's KiB comes
// from a binary search of aln_off that is the same for its 64 lanes, a lane's own from a few steps forward (else its own search),
// the place in the record's exception list from a search (sam_cursor_at); from there the 16 columns walk forward, over record borders
// too.  SEQ comes through an 8-byte window: 16 columns are two or three loads.
// small[]: SAMS_BAD records that are bad, SAMS_FIRST the smallest index of one (preset to ~0).
// ---------------------------------------------------------------------------------------------------------
enum { SAMS_BAD = 0, SAMS_FIRST = 1, SAMS_WORDS = 2 };
#define NS_SAM_WORD 16u
__global__ void __launch_bounds__(256) k_sam_scan(const uint8_t *__restrict__ cigar, const uint64_t *__restrict__ cigar_off, const uint8_t *__restrict__ md,
                                                  const uint64_t *__restrict__ md_off, const uint8_t *__restrict__ seq, const uint64_t *__restrict__ seq_off,
                                                  uint32_t n_aln, ns_sam_aln *__restrict__ aln, uint64_t *__restrict__ cols,
                                                  uint32_t *__restrict__ n_exc, SamExc *__restrict__ exc, unsigned long long *__restrict__ small) {
    const uint64_t a = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n_aln) return;
    const uint64_t sn = seq_off[a + 1] - seq_off[a];
    CsBytes cb(cigar + cigar_off[a]), mb(md + md_off[a]);
    SamFigures F;
    const bool ok = sam_scan_record(cb, cigar_off[a + 1] - cigar_off[a], mb, md_off[a + 1] - md_off[a], sn, sn == 1u && seq[seq_off[a]] == '*',
                                    exc + sam_exc_base(cigar_off, md_off, a), F);
    aln[a] = ns_sam_aln{F.head, F.tail, F.ref_len, F.query_len};
    cols[a] = F.cols; n_exc[a] = F.n_exc;
    if (!ok) { atomicAdd(&small[SAMS_BAD], 1ull); atomicMin(&small[SAMS_FIRST], (unsigned long long)a); }
}
__global__ void __launch_bounds__(256) k_sam_lines(const uint8_t *__restrict__ md, const uint64_t *__restrict__ md_off, const uint8_t *__restrict__ seq,
                                                   const uint64_t *__restrict__ seq_off, const uint64_t *__restrict__ cigar_off,
                                                   const ns_sam_aln *__restrict__ aln, const uint32_t *__restrict__ n_exc, const SamExc *__restrict__ exc,
                                                   const uint64_t *__restrict__ off, uint32_t n_aln,
                                                   uint8_t *__restrict__ ref_out, uint8_t *__restrict__ qry_out) {
    const uint64_t n_bytes = off[n_aln];
    const uint64_t g = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * NS_SAM_WORD;
    if (g >= n_bytes) return;
    uint32_t a = qual_locate(off, 0u, n_aln, g - (uint64_t)(threadIdx.x & 63u) * NS_SAM_WORD);      // (g < n_bytes: there is one)
    for (uint32_t s = 0; s < 4u && off[a + 1u] <= g; ++s) ++a;
    if (off[a + 1u] <= g) a = qual_locate(off, a + 1u, n_aln, g);
    uint64_t lo = off[a], hi = off[a + 1u];
    const SamExc *x = exc + sam_exc_base(cigar_off, md_off, a);
    uint32_t nx = n_exc[a];
    uint64_t seq_at = seq_off[a] + aln[a].head, md_at = md_off[a];
    SamCursor k;
    sam_cursor_at(k, x, nx, (uint32_t)(g - lo));
    CsBytes sb(seq), mb(md);
    uint32_t rw[4] = {0u, 0u, 0u, 0u}, qw[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (uint32_t b = 0; b < NS_SAM_WORD; ++b) {
        const uint64_t pos = g + b;
        if (pos < n_bytes) {
            if (pos >= hi) {                                  // the next record that has a column: its first one
                do ++a; while (off[a + 1u] <= pos);
                lo = off[a]; hi = off[a + 1u];
                x = exc + sam_exc_base(cigar_off, md_off, a); nx = n_exc[a];
                seq_at = seq_off[a] + aln[a].head; md_at = md_off[a];
                sam_cursor_at(k, x, nx, 0u);
            }
            uint8_t r, q;
            sam_column(k, x, nx, (uint32_t)(pos - lo), sb, seq_at, mb, md_at, r, q);
            rw[b >> 2] |= (uint32_t)r << (8u * (b & 3u));
            qw[b >> 2] |= (uint32_t)q << (8u * (b & 3u));
        }
    }
    *reinterpret_cast<uint4 *>(ref_out + g) = make_uint4(rw[0], rw[1], rw[2], rw[3]);
    *reinterpret_cast<uint4 *>(qry_out + g) = make_uint4(qw[0], qw[1], qw[2], qw[3]);
}

// ---------------------------------------------------------------------------------------------------------
// k_mixfit: the Nelder-Mead searches of the error-length mixtures (ns_mixfit.h; src/model_fitting.py:48-105), ONE WAVEFRONT PER START,
// four per workgroup.  The simplex, its values and every decision of the search are the same in all 64 lanes (each lane carries them in
// its own registers and takes the same branches); the lanes differ only inside an objective evaluation, where lane j has bin 64 t + j of
// tile t: the scan of the mismatch CDF and the maximum are cross-lane operations in the order ns_mixfit.h fixes.  The empirical CDF and
// the ln x! table (at most 8 KB each at the 1 000 bins a histogram can have) are read-only and shared by every wavefront: they come from
// global memory through the caches, there is no LDS and no barrier.  Searches end after different numbers of evaluations: whole
// wavefronts leave early, none diverges inside.  (One search per THREAD would put the 9 216 starts of an indel grid on 144 wavefronts of
// a device that holds 8 192, with 64 different trip counts in each.)
// ---------------------------------------------------------------------------------------------------------
#define NS_MF_WAVES 4u
template <class Obj>
__global__ void __launch_bounds__(256) k_mixfit(const double *__restrict__ cdf, const double *__restrict__ lnf, uint32_t n_bins,
                                                const double *__restrict__ starts, uint32_t n_starts, int evaluate, ns_mixfit_fit *__restrict__ out) {
    const uint32_t start = blockIdx.x * NS_MF_WAVES + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (start >= n_starts) return;                            // (the whole wavefront)
    const Obj obj{cdf, lnf, n_bins};
    const double *x0 = starts + (size_t)start * Obj::N;
    ns_mixfit_fit r;
    r.reserved = 0;
    if (evaluate) mf_evaluate(obj, x0, r);
    else mf_nelder_mead(obj, x0, 200u * Obj::N, 200u * Obj::N, r);
    if ((threadIdx.x & 63u) == 0) out[start] = r;
}

// ---------------------------------------------------------------------------------------------------------
// k_len_scan, k_len_flag, k_len_reduce: the lengths behind the read-length models (ns_read_len.h; src/head_align_tail_dist.py:134-229).
// SCAN, one record per thread, visited by descending CIGAR length as k_cs_hist: the CIGAR through an 8-byte CsBytes window; it writes the
// record's six figures (all zero for a bad record).  FLAG, one record per thread: the record's read comes from a binary search of
// read_off; whether it starts a segment depends on the figures of the read's first record and on the reference of the record in front
// of it, which SCAN has written — hence a kernel of its own.  The exclusive scan of the flags numbers the segments in record order:
// record a lies in segment seg[a] + flag[a] - 1.  REDUCE, one record per thread: ref_len is added to its segment, read_len / head / tail
// go to its read by atomic max / min, a flag counts a segment of its read.  Integers only: the order of the atomics does not show.
// reads[] is preset by the host side: read_len 0, head / tail = the read's extra_head / extra_tail (NS_LEN_NONE without), n_segments 0.
// small[]: LENS_BAD records that are bad, LENS_FIRST the smallest index of one (preset to ~0).
// ---------------------------------------------------------------------------------------------------------
enum { LENS_BAD = 0, LENS_FIRST = 1, LENS_WORDS = 2 };
__global__ void __launch_bounds__(256) k_len_scan(const uint8_t *__restrict__ cigar, const uint64_t *__restrict__ cigar_off, const uint8_t *__restrict__ reverse,
                                                  const uint32_t *__restrict__ ref_id, const uint64_t *__restrict__ ref_start,
                                                  const uint64_t *__restrict__ ref_total, uint32_t n_aln, const uint32_t *__restrict__ order,
                                                  ns_len_aln *__restrict__ aln, unsigned long long *__restrict__ small) {
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= n_aln) return;
    const uint64_t a = order ? order[tid] : tid;
    CsBytes cb(cigar + cigar_off[a]);
    LenFigures F;
    const bool ok = len_scan_record(cb, cigar_off[a + 1] - cigar_off[a], reverse[a] != 0, ref_start[a], ref_total[ref_id[a]], F);      // (ref_id < n_refs: the host checks)
    aln[a] = ns_len_aln{F.head, F.tail, F.read_len, F.ref_len, F.query_aln_len, F.edge};
    if (!ok) { atomicAdd(&small[LENS_BAD], 1ull); atomicMin(&small[LENS_FIRST], (unsigned long long)a); }
}
__global__ void __launch_bounds__(256) k_len_flag(const ns_len_aln *__restrict__ aln, const uint32_t *__restrict__ ref_id, const uint64_t *__restrict__ read_off,
                                                  uint32_t n_reads, uint32_t n_aln, int mode, uint32_t *__restrict__ rec_read, uint32_t *__restrict__ flag) {
    const uint32_t a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n_aln) return;
    const uint32_t r = qual_locate(read_off, 0u, n_reads, a);            // (read_off ends at n_aln: there is one)
    const uint64_t first = read_off[r];
    const bool is_first = first == a;
    rec_read[a] = r;
    flag[a] = len_starts_segment(mode, is_first, !is_first && ref_id[a - 1u] == ref_id[a], aln[first].edge, aln[a].edge) ? 1u : 0u;
}
__global__ void __launch_bounds__(256) k_len_reduce(const ns_len_aln *__restrict__ aln, const uint32_t *__restrict__ rec_read, const uint32_t *__restrict__ flag,
                                                    const uint32_t *__restrict__ seg, uint32_t n_aln, ns_len_read *__restrict__ reads,
                                                    unsigned long long *__restrict__ segments) {
    const uint32_t a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n_aln) return;
    const ns_len_aln A = aln[a];
    const uint32_t f = flag[a];
    ns_len_read *R = reads + rec_read[a];
    atomicAdd(&segments[seg[a] + f - 1u], (unsigned long long)A.ref_len);      // (record 0 has a flag: seg[a] + f >= 1, and <= n_aln)
    atomicMax(&R->read_len, A.read_len);
    atomicMin(&R->head, A.head);
    atomicMin(&R->tail, A.tail);
    if (f) atomicAdd(&R->n_segments, 1u);
}

// ---------------------------------------------------------------------------------------------------------
// k_chim_scan, k_chim_select: the split-alignment choice of chimeric reads (ns_chimeric.h; src/get_primary_sam.py:273-395).
// SCAN, one CIGAR per thread, visited by descending length as k_len_scan, through an 8-byte CsBytes window: the four figures of
// cigar_parser, or — where pysam[a] is set: the primary alignment of a read — of pysam (all zero for a bad CIGAR).
// SELECT, one read per thread, visited by descending number of entries (the same key and sort over ent_off): almost every read has no
// SA entry or one or two, and a wavefront's trip count is that of its longest read.  The lists of a read are bit masks in its slice of
// `ws` (ws_off[r], laid out by the host side from ent_off); its pieces go to the slice of `pieces` that starts at ent_off[r].  Every
// lane stays to the end: n_gaps and pos_strand are summed over the wavefront and leave in one 64-bit atomic each; species_count takes
// an atomic per recorded gap (chimeric reads are a few percent of a training set).  Integers only: the order of the atomics never shows.
// small[]: CHIMS_BAD CIGARs that are bad, CHIMS_FIRST the smallest index of one (preset to ~0), CHIMS_GAPS, CHIMS_POS the totals.
// ---------------------------------------------------------------------------------------------------------
enum { CHIMS_BAD = 0, CHIMS_FIRST = 1, CHIMS_GAPS = 2, CHIMS_POS = 3, CHIMS_WORDS = 4 };
__global__ void __launch_bounds__(256) k_chim_scan(const uint8_t *__restrict__ cigar, const uint64_t *__restrict__ cigar_off, uint32_t n,
                                                   const uint32_t *__restrict__ order, const uint8_t *__restrict__ pysam, ns_chim_ent *__restrict__ ent,
                                                   unsigned long long *__restrict__ small) {
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= n) return;
    const uint64_t a = order ? order[tid] : tid;
    CsBytes cb(cigar + cigar_off[a]);
    ChimFigures F;
    const bool ok = chim_scan_cigar(cb, cigar_off[a + 1] - cigar_off[a], pysam && pysam[a] ? CHIM_PYSAM : CHIM_PARSER, F);
    ent[a] = ns_chim_ent{F.qstart, F.qend, F.qlen, F.rlen};
    if (!ok) { atomicAdd(&small[CHIMS_BAD], 1ull); atomicMin(&small[CHIMS_FIRST], (unsigned long long)a); }
}
struct ChimAtomicAdd {
    __device__ __forceinline__ void operator()(unsigned long long *p, unsigned long long v) const { atomicAdd(p, v); }
};
__global__ void __launch_bounds__(256) k_chim_select(const ns_chim_ent *__restrict__ ent, const uint64_t *__restrict__ ent_off, uint32_t n_reads,
                                                     const uint32_t *__restrict__ order, const uint32_t *__restrict__ ref_id,
                                                     const uint64_t *__restrict__ ref_start, const uint32_t *__restrict__ nm,
                                                     const uint8_t *__restrict__ reverse, const uint64_t *__restrict__ ref_total,
                                                     const uint32_t *__restrict__ species, uint64_t *__restrict__ ws, const uint64_t *__restrict__ ws_off,
                                                     ns_chim_piece *__restrict__ pieces, ns_chim_read *__restrict__ reads,
                                                     unsigned long long *__restrict__ species_count, unsigned long long *__restrict__ small) {
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    ChimTotals T{0u, 0u};
    if (tid < n_reads) {
        const uint64_t r = order ? order[tid] : tid;
        const uint64_t e0 = ent_off[r];
        ChimAtomicAdd add;
        uint32_t flags = 0;
        static_assert(sizeof(ChimFigures) == sizeof(ns_chim_ent) && sizeof(ChimPiece) == sizeof(ns_chim_piece), "ns_chimeric.h mirrors the ABI structs");
        const uint32_t k = chim_select_read(ent_off[r + 1] - e0, reinterpret_cast<const ChimFigures *>(ent) + e0, ref_id + e0, ref_start + e0, nm + e0,
                                            reverse + e0, ref_total, species, ws + ws_off[r], reinterpret_cast<ChimPiece *>(pieces) + e0, species_count,
                                            add, T, flags);
        reads[r] = ns_chim_read{k, flags};
    }
    // (every lane of the workgroup comes here: the wavefront sums need them all)
    const unsigned long long gaps = wave_sum(T.n_gaps), pos = wave_sum(T.pos_strand);
    if ((threadIdx.x & 63u) == 0) {
        if (gaps) atomicAdd(&small[CHIMS_GAPS], gaps);
        if (pos) atomicAdd(&small[CHIMS_POS], pos);
    }
}

// ---------------------------------------------------------------------------------------------------------
// k_em_estep, k_em_accum, k_em_stop: one iteration of the quantification EM (ns_em.h; src/get_primary_sam.py:64-84, 108-127), bit for
// bit in the reference's summation order.  ESTEP, one multi-mapping item per thread: a gather, a divide and a multiply per candidate;
// the products go to slots that the host side laid out once per call, contiguous per target and ordered as the reference adds them.
// ACCUM, one wavefront per target, grid-stride: the ordered fold of the target's slots onto unique[t] — a serial chain of dependent fp64
// adds per target, which is the price of bit-identity —, then count[t], the new a[t] and dabs[t] = |new - old|.  STOP, one workgroup:
// wavefront 0 folds dabs[] in target order — the other serial chain, over every expressed target — while the other three take the
// minimum of a[] and count the non-finite ones; then one lane decides.  State (stop flag, iteration number, diff) stays on the device: the three kernels do nothing once the flag is set, so
// the host enqueues iterations in groups and reads the flag once per group.  No atomics on doubles anywhere.
// ---------------------------------------------------------------------------------------------------------
#define NS_EM_WAVES 4u
__global__ void __launch_bounds__(256) k_em_estep(const EmState *__restrict__ S, const double *__restrict__ a, const uint32_t *__restrict__ target,
                                                  const uint64_t *__restrict__ slot, const uint64_t *__restrict__ multi_off,
                                                  const double *__restrict__ weight, uint32_t n_multi, double *__restrict__ contrib) {
    if (S->stop) return;
    const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n_multi) return;
    em_item_estep(a, target, slot, multi_off[m], multi_off[m + 1], weight[m], contrib);
}
__global__ void __launch_bounds__(256) k_em_accum(const EmState *__restrict__ S, const double *__restrict__ contrib, const uint64_t *__restrict__ tgt_off,
                                                  const double *__restrict__ unique, double total, uint32_t n_targets,
                                                  double *__restrict__ count, double *__restrict__ a, double *__restrict__ dabs) {
    if (S->stop) return;
    const uint32_t wave = blockIdx.x * NS_EM_WAVES + (threadIdx.x >> 6), n_waves = gridDim.x * NS_EM_WAVES;
    for (uint32_t t = wave; t < n_targets; t += n_waves) {                // (the whole wavefront)
        const uint64_t lo = tgt_off[t];
        const double acc = em_fold(unique[t], contrib + lo, tgt_off[t + 1] - lo);
        if ((threadIdx.x & 63u) == 0) em_target_step(acc, total, count + t, a + t, dabs + t);
    }
}
__global__ void __launch_bounds__(256) k_em_stop(EmState *__restrict__ S, const double *__restrict__ a, const double *__restrict__ dabs, uint32_t n_targets,
                                                 double factor, uint32_t max_iter, double *__restrict__ diff_trace) {
    __shared__ double mn_s[256];
    __shared__ unsigned long long bad_s;
    if (S->stop) return;
    if (threadIdx.x == 0) bad_s = 0ull;
    __syncthreads();
    double mn = a[0], diff_tmp = 0.0;                                     // (n_targets >= 1: the host checks)
    if (threadIdx.x < 64u) diff_tmp = em_fold(0.0, dabs, n_targets);      // wavefront 0: the chain
    else {                                                                // the others, meanwhile: the minimum and the non-finite ones
        uint32_t bad = 0;
        for (uint32_t t = threadIdx.x - 64u; t < n_targets; t += blockDim.x - 64u) {
            const double v = a[t];
            mn = v < mn ? v : mn;
            if (!em_finite(v)) ++bad;
        }
        if (bad) atomicAdd(&bad_s, (unsigned long long)bad);
    }
    mn_s[threadIdx.x] = mn;
    __syncthreads();
    if (threadIdx.x >= 64u) return;
    for (uint32_t i = threadIdx.x + 64u; i < 256u; i += 64u) mn = mn_s[i] < mn ? mn_s[i] : mn;
    for (int o = 32; o > 0; o >>= 1) { const double u = __shfl_xor(mn, o, 64); mn = u < mn ? u : mn; }
    if (threadIdx.x == 0) em_decide(S, diff_tmp, mn, bad_s, factor, max_iter, diff_trace);
}

// ---------------------------------------------------------------------------------------------------------
// k_ir_walk: the Markov counts of the intron-retention model (ns_ir_train.h; src/model_intron_retention.py:104-176), one read per
// thread, visited by descending CIGAR length as k_len_scan, through an 8-byte CsBytes window.  A read marks the introns it retains in
// its own bit row (rows + row_off[r], ir_row_words(introns of its transcript) words, zeroed by the caller: a read can retain every
// intron of its transcript, and no list of fixed size stands between it and that), counts from the row, and ORs the row into the
// bitmap over all introns — the row's bit 0 is bit intr_off[t] there, so a word of the row goes to two words of the bitmap (which has
// one word to spare).  The six counters are privatised per workgroup in LDS and leave in one 64-bit atomic each.  A bad CIGAR leaves
// state 0, no count and no bit.  Integers only: the order of the atomics never shows.
// small[]: IRS_BAD CIGARs that are bad, IRS_FIRST the smallest index of one (preset to ~0), IRS_COUNT the six counts (IRC_*).
// ---------------------------------------------------------------------------------------------------------
enum { IRS_BAD = 0, IRS_FIRST = 1, IRS_COUNT = 2, IRS_WORDS = IRS_COUNT + IRC_WORDS };
__global__ void __launch_bounds__(256) k_ir_walk(const uint8_t *__restrict__ cigar, const uint64_t *__restrict__ cigar_off, const uint32_t *__restrict__ start,
                                                 const uint32_t *__restrict__ chrom, const uint32_t *__restrict__ trx, uint32_t n_reads,
                                                 const uint32_t *__restrict__ order, IrTables T, uint32_t *__restrict__ rows,
                                                 const uint64_t *__restrict__ row_off, uint32_t *__restrict__ bitmap, uint8_t *__restrict__ state,
                                                 unsigned long long *__restrict__ small) {
    __shared__ unsigned long long cnt[IRC_WORDS];
    if (threadIdx.x < IRC_WORDS) cnt[threadIdx.x] = 0ull;
    __syncthreads();
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid < n_reads) {
        const uint64_t r = order ? order[tid] : tid;
        const uint32_t t = trx[r];
        const IrTrx X = ir_trx(T, t);                              // (trx < n_trx or NS_IR_NONE: the host checks)
        uint32_t *row = rows + row_off[r];
        CsBytes cb(cigar + cigar_off[r]);
        bool ir_info;
        uint32_t st = IR_READ_NONE;
        if (ir_walk_read(cb, cigar_off[r + 1] - cigar_off[r], start[r], chrom[r], X, row, ir_info)) {
            unsigned long long c[IRC_WORDS] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
            st = ir_markov_read(X.n, row, ir_info, c);
            for (uint32_t i = 0; i < IRC_WORDS; ++i) if (c[i]) atomicAdd(&cnt[i], c[i]);
            if (st == IR_READ_IR) {
                const uint64_t bit0 = T.intr_off[t];
                for (uint64_t w = 0, nw = ir_row_words(X.n); w < nw; ++w) {
                    const uint32_t v = row[w];
                    if (!v) continue;
                    const uint64_t bit = bit0 + 32u * w;
                    const uint32_t sh = (uint32_t)(bit & 31u);
                    atomicOr(&bitmap[bit >> 5], v << sh);
                    if (sh && (v >> (32u - sh))) atomicOr(&bitmap[(bit >> 5) + 1u], v >> (32u - sh));
                }
            }
        } else { atomicAdd(&small[IRS_BAD], 1ull); atomicMin(&small[IRS_FIRST], (unsigned long long)r); }
        state[r] = (uint8_t)st;
    }
    __syncthreads();
    if (threadIdx.x < IRC_WORDS && cnt[threadIdx.x]) atomicAdd(&small[IRS_COUNT + threadIdx.x], cnt[threadIdx.x]);
}

// ---------------------------------------------------------------------------------------------------------
// k_maf_line_count, k_maf_line_write, k_maf_fields, k_maf_choose, k_maf_result, k_maf_emit, k_maf_names: the best hit per read of a MAF
// file (ns_maf_best.h; src/get_besthit_maf.py:8-56), from the bytes of the file.
// LINE_COUNT / LINE_WRITE: a workgroup looks at MAF_LINE_SPAN consecutive bytes of the text, a thread at 64 of them through an 8-byte
// window, and counts the `s`-line starts among them (the test looks one byte back and one ahead, over the span's border too: a span
// knows nothing else about its neighbours, and where a line ENDS is not its business — a line of 60 kb crosses four spans and is one
// start in the first).  The exclusive scan of the workgroups' counts (hipcub, between the two) says where a workgroup's starts go; WRITE
// repeats the test and places them by a scan over the workgroup: the starts are 64-bit offsets in the order of the text.
// FIELDS, one line per thread: maf_parse_line to the line's '\n'; the smallest index of a bad line by atomic min.
// CHOOSE, one pair per thread: maf_claim — the owner words only through atomicCAS — and maf_offer, one 64-bit atomicMax; the pair's slot
// goes to slot_of.  No loop waits for another thread; the probe walk is bounded by the table (MAFS_FULL if it ever ends there).
// RESULT, one pair per thread, in the NEXT kernel (the table is settled by the kernel boundary): kept iff the slot's key names the pair;
// num_aligned and pos_strand are summed per wavefront, then per workgroup in LDS, and leave in one atomic each per workgroup.
// EMIT, one pair per thread, behind the exclusive scan of the kept flags: the three records of a kept pair at its rank, in file order.
// NAMES, one name of the reads file per thread: maf_find in the settled table.
// small[]: MAFS_FIRST_BAD the smallest index of a bad line (preset to ~0), MAFS_ALIGNED, MAFS_POS, MAFS_FULL.
// ---------------------------------------------------------------------------------------------------------
enum { MAFS_FIRST_BAD = 0, MAFS_ALIGNED = 1, MAFS_POS = 2, MAFS_FULL = 3, MAFS_WORDS = 4 };
static_assert(MAF_LINE_SPAN == 256u * MAF_LINE_PER_THREAD, "a workgroup of the line kernels is 256 threads");
struct MafDevOps {
    __device__ __forceinline__ uint32_t cas(uint32_t *w, uint32_t expected, uint32_t desired) const { return atomicCAS(w, expected, desired); }
    __device__ __forceinline__ void max64(unsigned long long *w, unsigned long long v) const { atomicMax(w, v); }
};
// the `s`-line starts among a thread's 64 bytes as a bit mask
__device__ __forceinline__ uint64_t maf_thread_starts(const uint8_t *__restrict__ text, uint64_t nbytes) {
    const uint64_t b0 = (uint64_t)blockIdx.x * MAF_LINE_SPAN + (uint64_t)threadIdx.x * MAF_LINE_PER_THREAD;
    uint64_t mask = 0;
    if (b0 >= nbytes) return 0;
    CsBytes t(text), side(text);                                  // (`side`: the bytes in front of and behind a candidate keep their own window)
    for (uint32_t k = 0; k < MAF_LINE_PER_THREAD; ++k) {
        const uint64_t i = b0 + k;
        if (i + 1u >= nbytes) break;                              // (a start has a byte behind it)
        if (t[i] == 's' && maf_is_start(side, nbytes, i)) mask |= 1ull << k;
    }
    return mask;
}
__global__ void __launch_bounds__(256) k_maf_line_count(const uint8_t *__restrict__ text, uint64_t nbytes, unsigned long long *__restrict__ wg_count) {
    __shared__ unsigned long long part[4];
    const unsigned long long n = wave_sum((unsigned long long)__popcll(maf_thread_starts(text, nbytes)));
    if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) wg_count[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}
__global__ void __launch_bounds__(256) k_maf_line_write(const uint8_t *__restrict__ text, uint64_t nbytes, const unsigned long long *__restrict__ wg_base,
                                                        uint64_t n_lines, uint64_t *__restrict__ starts) {
    __shared__ uint32_t part[4];
    uint64_t mask = maf_thread_starts(text, nbytes);
    const uint32_t mine = (uint32_t)__popcll(mask), lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t incl = mine;                                          // the inclusive scan over the wavefront
    for (int o = 1; o < 64; o <<= 1) { const uint32_t u = (uint32_t)__shfl_up((int)incl, o, 64); if (lane >= (uint32_t)o) incl += u; }
    if (lane == 63u) part[wave] = incl;
    __syncthreads();
    uint64_t at = wg_base[blockIdx.x] + (incl - mine);
    for (uint32_t w = 0; w < wave; ++w) at += part[w];
    const uint64_t b0 = (uint64_t)blockIdx.x * MAF_LINE_SPAN + (uint64_t)threadIdx.x * MAF_LINE_PER_THREAD;
    while (mask) {
        const uint32_t k = (uint32_t)__ffsll((unsigned long long)mask) - 1u;
        mask &= mask - 1u;
        if (at < n_lines) starts[at] = b0 + k;                     // (at < n_lines: the count kernel saw the same bytes)
        ++at;
    }
}
__global__ void __launch_bounds__(256) k_maf_fields(const uint8_t *__restrict__ text, uint64_t nbytes, const uint64_t *__restrict__ starts, uint64_t n_lines,
                                                    MafLine *__restrict__ lines, unsigned long long *__restrict__ small) {
    const uint64_t l = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= n_lines) return;
    CsBytes t(text);
    MafLine L;
    const bool ok = maf_parse_line(t, nbytes, starts[l], L);
    lines[l] = L;
    if (!ok) atomicMin(&small[MAFS_FIRST_BAD], (unsigned long long)l);
}
__global__ void __launch_bounds__(256) k_maf_choose(const uint8_t *__restrict__ text, const MafLine *__restrict__ lines, uint32_t n_pairs, MafTable T,
                                                    uint32_t *__restrict__ slot_of, unsigned long long *__restrict__ small) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pairs) return;
    CsBytes t(text), u(text);
    const MafLine Q = lines[2ull * p + 1u];
    MafDevOps ops;
    uint64_t slot = maf_claim(t, u, lines, T, p, Q, ops);
    if (slot >= T.slots) { atomicAdd(&small[MAFS_FULL], 1ull); slot = 0; }
    else maf_offer(T, slot, p, Q.size, ops);
    slot_of[p] = (uint32_t)slot;                                   // (slots <= 2^32: a slot fits)
}
__global__ void __launch_bounds__(256) k_maf_result(const uint8_t *__restrict__ text, const MafLine *__restrict__ lines, uint32_t n_pairs, MafTable T,
                                                    const uint32_t *__restrict__ slot_of, uint32_t *__restrict__ flag, unsigned long long *__restrict__ small) {
    __shared__ unsigned long long cnt[2];
    if (threadIdx.x < 2u) cnt[threadIdx.x] = 0ull;
    __syncthreads();
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t kept = 0, pos = 0;
    if (p < n_pairs) {
        kept = maf_kept(T, slot_of[p], p) ? 1u : 0u;
        flag[p] = kept;
        if (kept) {
            CsBytes t(text), u(text);
            const MafLine R = lines[2ull * p], Q = lines[2ull * p + 1u];
            pos = maf_same_bytes(t, R.strand_at, R.strand_len, u, Q.strand_at, Q.strand_len) ? 1u : 0u;
        }
    }
    // (every lane of the workgroup comes here: the wavefront sums need them all)
    const unsigned long long k = wave_sum((unsigned long long)kept), s = wave_sum((unsigned long long)pos);
    if ((threadIdx.x & 63u) == 0) { if (k) atomicAdd(&cnt[0], k); if (s) atomicAdd(&cnt[1], s); }
    __syncthreads();
    if (threadIdx.x == 0) { if (cnt[0]) atomicAdd(&small[MAFS_ALIGNED], cnt[0]); if (cnt[1]) atomicAdd(&small[MAFS_POS], cnt[1]); }
}
__global__ void __launch_bounds__(256) k_maf_emit(uint64_t nbytes, const uint64_t *__restrict__ starts, const MafLine *__restrict__ lines, uint32_t n_pairs,
                                                  const uint32_t *__restrict__ flag, const uint32_t *__restrict__ rank, MafOutLines *__restrict__ out_lines,
                                                  MafOutRecord *__restrict__ out_records, MafOutFigures *__restrict__ out_figures) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pairs || !flag[p]) return;
    const uint32_t k = rank[p];                                    // (< the number of kept pairs <= n_pairs: the arrays hold n_pairs)
    const MafLine R = lines[2ull * p], Q = lines[2ull * p + 1u];
    maf_emit(nbytes, starts[2ull * p], R, starts[2ull * p + 1u], Q, out_lines[k], out_records[k], out_figures[k]);
}
__global__ void __launch_bounds__(256) k_maf_names(const uint8_t *__restrict__ text, const MafLine *__restrict__ lines, MafTable T,
                                                   const uint8_t *__restrict__ names, const uint64_t *__restrict__ names_off, uint32_t n_names,
                                                   uint8_t *__restrict__ found) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_names) return;
    CsBytes t(text), nb(names);
    const uint64_t lo = names_off[i], n = names_off[i + 1u] - lo;
    found[i] = n <= 0xffffffffull && maf_find(t, lines, T, nb, lo, (uint32_t)n) ? 1u : 0u;
}

// ---------------------------------------------------------------------------------------------------------
// k_sam_sep_count, k_sam_sep_write, k_sam_tags, k_sam_rows: the index of a SAM text (ns_sam_index.h), from the bytes of the file.
// SEP_COUNT / SEP_WRITE: a workgroup looks at SAM_SPAN consecutive bytes in SAM_LOADS loads; in load i lane t of the workgroup reads the
// 16 bytes at 4096 i + 16 t of the span, so that a wavefront's load instruction covers 1 KiB of consecutive text.  COUNT sums the '\n',
// the '\t' and the odd bytes of the span.  Behind the exclusive scans of the workgroups' two counts, WRITE repeats the masks and ranks
// every separator in the order of the TEXT, which is (load, lane, byte) and not (lane, byte): an inclusive scan over the wavefront per
// load, the wavefronts' totals per load in LDS, and a walk over the 16 totals.  The two counts travel packed in one word (16 bits each:
// a span has at most 16384 of either).  A '\n' writes the start of the line behind it with its tab rank and whether that line is a
// header line; a '\t' writes its position and its line (the number of '\n' in front of it).  Entry 0 and, behind a last line without
// '\n', the closing entry are thread 0's.
// TAGS, one tab per thread: sam_tag_offer, one atomicMax.  ROWS, one line per thread, in the NEXT kernel (the slots are settled by the
// kernel boundary) and behind the exclusive scan of the header flags: a record goes to row l - (headers in front of it), a header line
// to the header list.  small[]: SAMI_ODD, SAMI_CS, SAMI_MD (records with the tag), SAMI_LONG (lines of 2^32 bytes or more).
// ---------------------------------------------------------------------------------------------------------
enum { SAMI_ODD = 0, SAMI_CS = 1, SAMI_MD = 2, SAMI_LONG = 3, SAMI_WORDS = 4 };
static_assert(SAM_SPAN == 256u * SAM_CHUNK * SAM_LOADS && SAM_SPAN <= 0xffffu, "a workgroup of the separator kernels is 256 threads; a count fits 16 bits");
struct SamDevOps {
    __device__ __forceinline__ void max32(uint32_t *w, uint32_t v) const { atomicMax(w, v); }
};
// where chunk (load, thread) of this workgroup begins in the text, and its masks (none beyond the text)
__device__ __forceinline__ uint64_t sam_chunk_at(uint32_t load) {
    return (uint64_t)blockIdx.x * SAM_SPAN + (uint64_t)load * (256u * SAM_CHUNK) + (uint64_t)threadIdx.x * SAM_CHUNK;
}
__device__ __forceinline__ SamChunk sam_load_chunk(const uint8_t *__restrict__ text, uint64_t nbytes, uint32_t load) {
    const uint64_t at = sam_chunk_at(load);
    if (at >= nbytes) return SamChunk{0u, 0u, 0u};
    // (16-byte aligned: the text begins an allocation; its last chunk ends inside the NS_WINDOW_PAD bytes behind it)
    const uint4 v = *reinterpret_cast<const uint4 *>(text + at);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    return sam_chunk(w, nbytes - at >= SAM_CHUNK ? SAM_CHUNK : (uint32_t)(nbytes - at));
}
__global__ void __launch_bounds__(256) k_sam_sep_count(const uint8_t *__restrict__ text, uint64_t nbytes, unsigned long long *__restrict__ wg_nl,
                                                       unsigned long long *__restrict__ wg_tab, unsigned long long *__restrict__ small) {
    __shared__ unsigned long long part[4];
    unsigned long long n = 0;                                      // three counts of at most 2^14 each, 20 bits apart
    for (uint32_t i = 0; i < SAM_LOADS; ++i) {
        const SamChunk c = sam_load_chunk(text, nbytes, i);
        n += (unsigned long long)__popc(c.nl) | (unsigned long long)__popc(c.tab) << 20 | (unsigned long long)__popc(c.odd) << 40;
    }
    n = wave_sum(n);
    if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        n = part[0] + part[1] + part[2] + part[3];
        wg_nl[blockIdx.x] = n & 0xfffffull;
        wg_tab[blockIdx.x] = (n >> 20) & 0xfffffull;
        if (n >> 40) atomicAdd(&small[SAMI_ODD], n >> 40);
    }
}
__global__ void __launch_bounds__(256) k_sam_sep_write(const uint8_t *__restrict__ text, uint64_t nbytes, const unsigned long long *__restrict__ wg_nl_base,
                                                       const unsigned long long *__restrict__ wg_tab_base, uint64_t n_nl, uint64_t n_tabs, uint64_t n_lines,
                                                       uint64_t *__restrict__ line_start, uint64_t *__restrict__ line_rank, uint32_t *__restrict__ hdr_flag,
                                                       uint64_t *__restrict__ tab_pos, uint32_t *__restrict__ tab_line) {
    __shared__ uint32_t part[SAM_LOADS][4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    SamChunk c[SAM_LOADS];
    uint32_t excl[SAM_LOADS];                                      // packed: '\n' in the low half, '\t' in the high half
    for (uint32_t i = 0; i < SAM_LOADS; ++i) {
        c[i] = sam_load_chunk(text, nbytes, i);
        const uint32_t mine = (uint32_t)__popc(c[i].nl) | (uint32_t)__popc(c[i].tab) << 16;
        uint32_t incl = mine;                                      // the inclusive scan over the wavefront
        for (int o = 1; o < 64; o <<= 1) { const uint32_t u = (uint32_t)__shfl_up((int)incl, o, 64); if (lane >= (uint32_t)o) incl += u; }
        if (lane == 63u) part[i][wave] = incl;
        excl[i] = incl - mine;
    }
    __syncthreads();
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        CsBytes t(text);
        line_start[0] = 0; line_rank[0] = 0; hdr_flag[0] = sam_is_header(t, nbytes, 0) ? 1u : 0u;
        if (n_lines > n_nl) { line_start[n_lines] = nbytes + 1u; line_rank[n_lines] = n_tabs; }     // (the last line has no '\n')
    }
    const uint64_t nl_base = wg_nl_base[blockIdx.x], tab_base = wg_tab_base[blockIdx.x];
    uint32_t before = 0;                                           // the separators of the loads in front of load i
    CsBytes t(text);
    for (uint32_t i = 0; i < SAM_LOADS; ++i) {
        uint32_t in_front = before + excl[i];
        for (uint32_t w = 0; w < 4u; ++w) { if (w < wave) in_front += part[i][w]; before += part[i][w]; }
        const uint64_t at = sam_chunk_at(i), nl_at = nl_base + (in_front & 0xffffu), tab_at = tab_base + (in_front >> 16);
        for (uint32_t m = c[i].tab; m; m &= m - 1u) {
            const uint32_t k = (uint32_t)__ffs((int)m) - 1u;
            const uint64_t j = tab_at + (uint32_t)__popc(sam_below(c[i].tab, k));
            if (j < n_tabs) { tab_pos[j] = at + k; tab_line[j] = (uint32_t)(nl_at + (uint32_t)__popc(sam_below(c[i].nl, k))); }     // (j < n_tabs: the count kernel saw the same bytes)
        }
        for (uint32_t m = c[i].nl; m; m &= m - 1u) {
            const uint32_t k = (uint32_t)__ffs((int)m) - 1u;
            const uint64_t j = nl_at + (uint32_t)__popc(sam_below(c[i].nl, k)) + 1u;                  // the line behind this '\n'
            if (j <= n_nl) {
                line_start[j] = at + k + 1u;
                line_rank[j] = tab_at + (uint32_t)__popc(sam_below(c[i].tab, k));
                hdr_flag[j] = sam_is_header(t, nbytes, at + k + 1u) ? 1u : 0u;
            }
        }
    }
}
__global__ void __launch_bounds__(256) k_sam_tags(const uint8_t *__restrict__ text, SamLists L, const uint32_t *__restrict__ tab_line, uint64_t n_tabs,
                                                  uint32_t *__restrict__ slots) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_tabs) return;
    CsBytes t(text);
    SamDevOps ops;
    sam_tag_offer(t, L, i, tab_line[i], slots, ops);
}
__global__ void __launch_bounds__(256) k_sam_rows(const uint8_t *__restrict__ text, SamLists L, const uint32_t *__restrict__ slots,
                                                  const uint32_t *__restrict__ hdr_rank, SamRow *__restrict__ rows, SamSpan *__restrict__ header,
                                                  unsigned long long *__restrict__ small) {
    const uint64_t l = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long n = 0;                                      // SAMI_CS, SAMI_MD, SAMI_LONG, 20 bits apart
    if (l < L.n_lines) {
        CsBytes t(text);
        SamRow R; SamSpan H;
        const uint32_t h = hdr_rank[l];
        const int what = sam_row(t, L, l, slots, R, H);
        if (what == SAM_LINE_RECORD) {
            rows[l - h] = R;
            n = (R.bits & SAM_HAS_CS ? 1ull : 0ull) | (R.bits & SAM_HAS_MD ? 1ull << 20 : 0ull);
        } else if (what == SAM_LINE_HEADER) header[h] = H;
        else n = 1ull << 40;
    }
    // (every lane of the wavefront comes here: the sum needs them all)
    n = wave_sum(n);
    if ((threadIdx.x & 63u) == 0 && n) {
        if (n & 0xfffffull) atomicAdd(&small[SAMI_CS], n & 0xfffffull);
        if ((n >> 20) & 0xfffffull) atomicAdd(&small[SAMI_MD], (n >> 20) & 0xfffffull);
        if (n >> 40) atomicAdd(&small[SAMI_LONG], n >> 40);
    }
}

// ---------------------------------------------------------------------------------------------------------
// k_bam_measure, k_bam_float_len, k_bam_write: BAM records to SAM text (ns_bam.h), one wavefront per record (measure) and per slice of a
// record (write), four to a workgroup.
// MEASURE: bam_measure; the line's length without its floats, the number of its slices and what the write pass needs of it (BamRec);
// where a float stands goes to flt_at at a slot taken from small[BAMS_N_FLOAT] (beyond flt_cap it is only counted: the host runs the
// kernel again with a list that holds them all); the smallest (index << 8 | reason) of a bad record by atomic min.
// FLOAT_LEN, one record per thread, after the host has sorted the places, made the text of every float and found the first slot of
// every record: the characters of the record's floats are added to the length of its line.
// WRITE: wavefront g finds its record by bisection in the exclusive scan of the slice counts and writes slice g - slice_off[r] of it
// (bam_write) at line_off[r]; a line that is not what MEASURE measured counts in small[BAMS_MISMATCH].
// ---------------------------------------------------------------------------------------------------------
enum { BAMS_FIRST_BAD = 0, BAMS_N_FLOAT = 1, BAMS_MISMATCH = 2, BAMS_WORDS = 4 };
static_assert(BAM_ROUND_OPS == 64u && BAM_LANE_BYTES == sizeof(BamPiece) && BAM_SLICE_BASES % 2u == 0u, "a round is a wavefront, a piece one store");
struct BamWaveDev {
    static constexpr uint32_t LANES = 64u;
    uint32_t lane;
    unsigned long long *flt_at, *flt_n;
    uint64_t flt_cap;
    __device__ __forceinline__ uint32_t scan(uint32_t v, uint32_t &total) const {
        uint32_t incl = v;
        for (int o = 1; o < 64; o <<= 1) { const uint32_t u = (uint32_t)__shfl_up((int)incl, o, 64); if (lane >= (uint32_t)o) incl += u; }
        total = (uint32_t)__shfl((int)incl, 63, 64);
        return incl - v;
    }
    __device__ __forceinline__ uint32_t first(bool pred) const { const unsigned long long m = __ballot(pred); return m ? (uint32_t)__ffsll(m) - 1u : 64u; }
    __device__ __forceinline__ uint32_t bcast(uint32_t v, uint32_t src) const { return (uint32_t)__shfl((int)v, (int)src, 64); }
    __device__ __forceinline__ uint64_t float_reserve(uint32_t n) const {
        unsigned long long at = 0;
        if (lane == 0) at = atomicAdd(flt_n, (unsigned long long)n);
        return ((uint64_t)(uint32_t)__shfl((int)(at >> 32), 0, 64) << 32) | (uint32_t)__shfl((int)(uint32_t)at, 0, 64);
    }
    __device__ __forceinline__ void float_put(uint64_t slot, uint64_t where) const { if (slot < flt_cap) flt_at[slot] = where; }
};
__global__ void __launch_bounds__(256) k_bam_measure(const uint8_t *__restrict__ bytes, const uint64_t *__restrict__ rec_off, uint32_t n_rec, BamRefs R,
                                                     BamRec *__restrict__ rec, unsigned long long *__restrict__ line_len, uint32_t *__restrict__ slices,
                                                     unsigned long long *__restrict__ flt_at, uint64_t flt_cap, unsigned long long *__restrict__ small) {
    const uint32_t r = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (r >= n_rec) return;                                        // (a whole wavefront leaves)
    BamWaveDev w{threadIdx.x & 63u, flt_at, &small[BAMS_N_FLOAT], flt_cap};
    BamRec rc;
    uint64_t len = 0;
    uint32_t ns = 1;
    const uint32_t reason = bam_measure(w, bytes, rec_off[r], rec_off[r + 1u], R, rc, len, ns);
    if (w.lane) return;
    if (reason) { atomicMin(&small[BAMS_FIRST_BAD], ((unsigned long long)r << 8) | reason); return; }
    rec[r] = rc; line_len[r] = len; slices[r] = ns;
}
__global__ void __launch_bounds__(256) k_bam_float_len(const uint32_t *__restrict__ flt_first, const uint8_t *__restrict__ slots, uint32_t n_rec,
                                                       unsigned long long *__restrict__ line_len) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rec) return;
    unsigned long long add = 0;
    for (uint32_t k = flt_first[r]; k < flt_first[r + 1u]; ++k) { const uint32_t l = slots[(uint64_t)k * BAM_FLOAT_SLOT + BAM_FLOAT_SLOT - 1u]; add += l > BAM_FLOAT_CHARS ? BAM_FLOAT_CHARS : l; }
    if (add) line_len[r] += add;
}
__global__ void __launch_bounds__(256) k_bam_write(const uint8_t *__restrict__ bytes, const uint64_t *__restrict__ rec_off, uint32_t n_rec, BamRefs R,
                                                   const BamRec *__restrict__ rec, const unsigned long long *__restrict__ line_off,
                                                   const uint32_t *__restrict__ slice_off, uint32_t n_slices, const uint32_t *__restrict__ flt_first,
                                                   const uint8_t *__restrict__ slots, uint8_t *__restrict__ text, unsigned long long *__restrict__ small) {
    const uint32_t g = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (g >= n_slices) return;
    uint32_t lo = 0, hi = n_rec - 1u;                              // the last record whose first slice is not behind g
    while (lo < hi) { const uint32_t mid = lo + (hi - lo + 1u) / 2u; if (slice_off[mid] <= g) lo = mid; else hi = mid - 1u; }
    const uint32_t r = lo;
    BamWaveDev w{threadIdx.x & 63u, nullptr, nullptr, 0};
    const BamRec rc = rec[r];
    const uint64_t at = line_off[r];
    const bool ok = bam_write(w, bytes, rec_off[r], rec_off[r + 1u], R, rc, g - slice_off[r], flt_first ? slots + (uint64_t)flt_first[r] * BAM_FLOAT_SLOT : nullptr,
                              text + at, line_off[r + 1u] - at);
    if (!ok && w.lane == 0) atomicAdd(&small[BAMS_MISMATCH], 1ull);
}

// ---------------------------------------------------------------------------------------------------------
// k_calmd_measure, k_calmd_write: the MD and cs text of alignments from the reference genome (ns_calmd.h), one wavefront per record, four
// to a workgroup, in both.
// MEASURE: calmd_measure — the record is checked, its ops go to its table (at calmd_op_base), the lengths of its two texts to md_len and
// cs_len; a bad record has lengths 0, counts in small[CALMDS_N_BAD] and gives the smallest (index << 8 | reason) by atomic min.
// WRITE, after the exclusive scans of the lengths: calmd_text<true> at md_off[r] and cs_off[r]; a text that is not what MEASURE measured
// counts in small[CALMDS_MISMATCH].
// ---------------------------------------------------------------------------------------------------------
enum { CALMDS_FIRST_BAD = 0, CALMDS_N_BAD = 1, CALMDS_MISMATCH = 2, CALMDS_WORDS = 4 };
struct CalmdWaveDev {
    static constexpr uint32_t LANES = 64u;
    uint32_t lane;
    __device__ __forceinline__ uint64_t ballot(bool pred) const { return __ballot(pred); }
    __device__ __forceinline__ uint64_t scan(uint64_t v, uint64_t &total) const {
        uint64_t incl = v;
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)incl, o, 64), hi = (uint32_t)__shfl_up((int)(uint32_t)(incl >> 32), o, 64);
            if (lane >= (uint32_t)o) incl += ((uint64_t)hi << 32) | lo;
        }
        total = ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(incl >> 32), 63, 64) << 32) | (uint32_t)__shfl((int)(uint32_t)incl, 63, 64);
        return incl - v;
    }
    __device__ __forceinline__ uint32_t bcast(uint32_t v, uint32_t src) const { return (uint32_t)__shfl((int)v, (int)src, 64); }
    __device__ __forceinline__ void fence() const { __threadfence_block(); }
};
__global__ void __launch_bounds__(256) k_calmd_measure(const uint8_t *__restrict__ cigar, const uint64_t *__restrict__ cigar_off, const uint8_t *__restrict__ seq,
                                                       const uint64_t *__restrict__ seq_off, const uint32_t *__restrict__ chrom, const uint32_t *__restrict__ pos,
                                                       uint32_t n_rec, CalmdRef G, CalmdOp *ops, CalmdRec *__restrict__ rec,
                                                       unsigned long long *__restrict__ md_len, unsigned long long *__restrict__ cs_len,
                                                       unsigned long long *__restrict__ small) {
    const uint32_t r = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (r >= n_rec) return;                                        // (a whole wavefront leaves)
    CalmdWaveDev w{threadIdx.x & 63u};
    CalmdRec R;
    uint64_t ml = 0, cl = 0;
    const uint64_t c0 = cigar_off[r], s0 = seq_off[r];
    const uint32_t reason = calmd_measure(w, cigar + c0, cigar_off[r + 1u] - c0, seq + s0, seq_off[r + 1u] - s0, chrom[r], pos[r], G,
                                          ops + calmd_op_base(cigar_off, r), R, ml, cl);
    if (w.lane) return;
    rec[r] = R; md_len[r] = ml; cs_len[r] = cl;
    if (reason) { atomicMin(&small[CALMDS_FIRST_BAD], ((unsigned long long)r << 8) | reason); atomicAdd(&small[CALMDS_N_BAD], 1ull); }
}
__global__ void __launch_bounds__(256) k_calmd_write(const uint64_t *__restrict__ cigar_off, const uint8_t *__restrict__ seq, const uint64_t *__restrict__ seq_off,
                                                     const uint32_t *__restrict__ chrom, const uint32_t *__restrict__ pos, uint32_t n_rec, CalmdRef G,
                                                     const CalmdOp *__restrict__ ops, const CalmdRec *__restrict__ rec,
                                                     const unsigned long long *__restrict__ md_off, const unsigned long long *__restrict__ cs_off,
                                                     uint8_t *__restrict__ md, uint8_t *__restrict__ cs, unsigned long long *__restrict__ small) {
    const uint32_t r = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (r >= n_rec) return;
    const CalmdRec R = rec[r];
    if (R.reason) return;                                          // (MEASURE has checked chrom and POS of the others)
    CalmdWaveDev w{threadIdx.x & 63u};
    const uint64_t ma = md_off[r], ca = cs_off[r];
    uint64_t ml = 0, cl = 0;
    const bool ok = calmd_text<true>(w, ops + calmd_op_base(cigar_off, r), R, seq + seq_off[r], G.bases + G.chrom_off[chrom[r]] + (pos[r] - 1u), md + ma,
                                     md_off[r + 1u] - ma, cs + ca, cs_off[r + 1u] - ca, ml, cl);
    if (!ok && w.lane == 0) atomicAdd(&small[CALMDS_MISMATCH], 1ull);
}
