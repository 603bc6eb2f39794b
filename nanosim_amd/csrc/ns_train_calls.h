// ns_train_calls.h — training side, the host calls (their kernels are ns_train.h).  Not a translation unit of its own:
// nanosim_amd.hip includes it once, behind ns_ctx, fail, grow, with_tmp, scan_sum and free_pool, which it uses.  Every call reads the
// same way: check the arguments, a CallScratch with every buffer, upload(), begin(), the kernels, finish() (and fetch() wherever the host
// has to wait for a size in between), the results.  Nothing here is called by the simulator's driver.
#pragma once

struct ReadBack { void *dst; const void *src; size_t bytes; };                    // a copy to the host (bytes == 0: none)
struct DevStrings { const uint8_t *bytes; const uint64_t *off; };                 // strings one behind the other and their n + 1 offsets, on the device
// the bytes to spare behind strings on the device: the 8- and 16-byte window loads of CsBytes read past the last string
static const size_t NS_WINDOW_PAD = 16;

// The device memory of ONE training-side call (`call`: its public name, for the messages) and the call's operations on the main stream.
// The memory is a pool like those of upload(), taken per call and given back when the call returns, whichever way it returns: the
// destructor is the only place where this memory is freed.  (Not grow-only buffers of the context: the alignments of a training set are
// gigabytes, and the context simulates afterwards.)  A call asks for all of its buffers first and then has them filled (upload()): every
// allocation in front of the first copy, which keeps the host from mapping memory while the stream works.
// The first failure stays in `rc` (NS_ENOMEM for an allocation, a scan's own status, NS_EHIP otherwise; the message in the context) and
// turns what follows into no-ops (alloc returns nullptr, nothing more is launched): upload(), fetch() and finish() report it, and a call
// looks at nothing the device wrote before one of them has returned NS_OK.
struct CallScratch {
    struct Fill { void *dst; const void *src; size_t bytes; };                    // (src == nullptr: zeroes)
    ns_ctx *ctx; const char *call;
    int rc = NS_OK;
    std::vector<void *> pool;
    std::vector<Fill> fills;
    CallScratch(ns_ctx *c, const char *name) : ctx(c), call(name) {}
    CallScratch(const CallScratch &) = delete;
    ~CallScratch() { free_pool(pool); }
    int check(hipError_t e) {
        if (e != hipSuccess && !rc) rc = fail(ctx, NS_EHIP, std::string(call) + ": " + hipGetErrorString(e));
        return rc;
    }
    template <typename T> T *alloc(size_t n, size_t pad = 0) {                    // n elements + pad bytes, as they are
        void *p = nullptr;
        if (rc) return nullptr;
        const hipError_t e = hipMalloc(&p, n * sizeof(T) + pad);
        if (e != hipSuccess) {
            (void)hipGetLastError();             // the failed allocation must not poison the next call
            rc = fail(ctx, NS_ENOMEM, std::string(call) + ": hipMalloc: " + hipGetErrorString(e));
            return nullptr;
        }
        pool.push_back(p);
        return static_cast<T *>(p);
    }
    template <typename T> T *zeroed(size_t n, size_t pad = 0) {                   // ... the n elements zeroed by upload()
        T *p = alloc<T>(n, pad);
        if (p) fills.push_back({p, nullptr, n * sizeof(T)});
        return p;
    }
    template <typename T> T *filled(const T *src, size_t n, size_t pad = 0) {     // ... the n elements copied from the host by upload()
        T *p = alloc<T>(n, pad);
        if (p && n) fills.push_back({p, src, n * sizeof(T)});
        return p;
    }
    int upload() {                               // the copies and memsets asked for so far, on the main stream, in the order asked
        for (const Fill &f : fills)
            if (!rc) check(f.src ? hipMemcpyAsync(f.dst, f.src, f.bytes, hipMemcpyHostToDevice, ctx->stream) : hipMemsetAsync(f.dst, 0, f.bytes, ctx->stream));
        fills.clear();
        return rc;
    }
};
// The operations of a call on the main stream.  After a failure (s.rc) they do nothing; fetch() and finish() return it.
// strings one behind the other and, next on the stream, their n + 1 offsets, filled by upload()
static DevStrings strings(CallScratch &s, const uint8_t *bytes, uint64_t nbytes, const uint64_t *off, uint32_t n) {
    const uint8_t *d_bytes = s.filled(bytes, (size_t)nbytes, NS_WINDOW_PAD);
    return {d_bytes, s.filled(off, (size_t)n + 1)};
}
// the call's three events: begin() in front of the first kernel, finish() behind the last; mark() in between, for the calls that time a first part
static void record(CallScratch &s, Evt e) { if (!s.rc) s.check(hipEventRecord(s.ctx->evt[e], s.ctx->stream)); }
static int ms_to(CallScratch &s, Evt e, double *ms) {                            // (behind finish(): the stream is drained)
    float f = 0;
    if (!s.check(hipEventElapsedTime(&f, s.ctx->evt[EV_TRAIN_BEGIN], s.ctx->evt[e]))) *ms = f;
    return s.rc;
}
static int begin(CallScratch &s) { record(s, EV_TRAIN_BEGIN); return s.rc; }
static void mark(CallScratch &s) { record(s, EV_TRAIN_MID); }
static int ms_to_mark(CallScratch &s, double *ms) { return ms_to(s, EV_TRAIN_MID, ms); }
// a kernel.  The arguments convert to the kernel's parameter types as they would in a launch written out
template <typename... P> static void launch(CallScratch &s, void (*kernel)(P...), dim3 grid, dim3 block, std::common_type_t<P>... args) {
    if (s.rc) return;
    kernel<<<grid, block, 0, s.ctx->stream>>>(args...);
    s.check(hipGetLastError());
}
template <typename... P> static void per_thread(CallScratch &s, void (*kernel)(P...), uint64_t n, std::common_type_t<P>... args) {     // ... a thread per item, 256 per workgroup
    launch(s, kernel, dim3((unsigned)((n + 255u) / 256u)), dim3(256), args...);
}
template <typename T> static void scan(CallScratch &s, const T *in, T *out, size_t n) {      // scan_sum: its own status, the call's name in front of its message
    if (s.rc) return;
    if (int r = scan_sum(s.ctx, in, out, n)) s.rc = fail(s.ctx, r, std::string(s.call) + ": " + s.ctx->err);
}
static int fetch(CallScratch &s, std::initializer_list<ReadBack> back) {          // the copies to the host, and the stream drained: the host waits here
    for (const ReadBack &b : back)
        if (b.bytes && !s.rc) s.check(hipMemcpyAsync(b.dst, b.src, b.bytes, hipMemcpyDeviceToHost, s.ctx->stream));
    return s.rc ? s.rc : s.check(hipStreamSynchronize(s.ctx->stream));
}
static int finish(CallScratch &s, std::initializer_list<ReadBack> back, double *ms) {        // the end of a call: EV_TRAIN_END, fetch(); *ms = begin() .. here
    record(s, EV_TRAIN_END);
    return fetch(s, back) ? s.rc : ms_to(s, EV_TRAIN_END, ms);
}

// "ascending and not beyond the bytes" for the n + 1 offsets of a call's strings (`what`: what the message calls them)
static int check_offsets(ns_ctx *ctx, const char *call, const char *what, const uint64_t *off, uint32_t n, uint64_t nbytes) {
    for (uint32_t a = 0; a < n; ++a)
        if (off[a] > off[a + 1] || off[a + 1] > nbytes) return fail(ctx, NS_EINVAL, std::string(call) + ": offsets not ascending / beyond the " + what);
    return NS_OK;
}
// ... for strings whose size is their last offset: and there are bytes when that is not 0
static int check_strings(ns_ctx *ctx, const char *call, const char *what, const uint8_t *bytes, const uint64_t *off, uint32_t n) {
    if (int rc = check_offsets(ctx, call, what, off, n, off[n])) return rc;
    return !bytes && off[n] ? fail(ctx, NS_EINVAL, std::string(call) + ": null argument") : NS_OK;
}
// Alignments of 1 kb .. 100 kb on neighbouring lanes diverge like the thread-per-read chain did before its length sort: the walks are
// visited by descending length of their cs strings (the counts are sums: any order gives the same tables).  Returns the visiting order
// (nullptr for 64 alignments or fewer: index order — and after a failure, which stays in s.rc).  It lies in the key block, which is the
// call's; only the sort's temporary storage is the context's (with_tmp).  A later with_tmp of the same call (a scan) may regrow scan_tmp
// and free the storage the sort is still using on the stream: hipFree waits for the device, and nothing of the result is in there.
static uint32_t *order_by_length(CallScratch &s, const uint64_t *d_off, uint32_t n_aln) {
    if (n_aln <= 64) return nullptr;
    ns_ctx *ctx = s.ctx;
    uint32_t *key = s.alloc<uint32_t>((size_t)4 * n_aln);                 // key, index, sorted key, sorted index
    if (!key) return nullptr;
    uint32_t *idx = key + n_aln, *key2 = idx + n_aln, *idx2 = key2 + n_aln;
    per_thread(s, k_cs_len, n_aln, d_off, n_aln, key, idx);
    if (s.rc) return nullptr;
    if (int rc = with_tmp(ctx, "DeviceRadixSort::SortPairsDescending", [&](void *tmp, size_t &bytes) {
            return hipcub::DeviceRadixSort::SortPairsDescending(tmp, bytes, key, key2, idx, idx2, (int)n_aln, 0, 32, ctx->stream); }))
        s.rc = fail(ctx, rc, std::string(s.call) + ": " + ctx->err);
    return s.rc ? nullptr : idx2;
}
// The bad records of a walk.  Most walks keep {how many, the smallest index of one} in the first two words of their small block
// (SAMS_, LENS_, CHIMS_, IRS_BAD and _FIRST): bad_preset is what their atomics start from, bad_count the read-out (n: the index without
// one).  The walks that say why keep the smallest `index << 8 | reason` (BAMS_, CALMDS_FIRST_BAD, preset to ~0): bad_unpack
static_assert(SAMS_BAD == 0 && SAMS_FIRST == 1 && LENS_BAD == 0 && LENS_FIRST == 1 && CHIMS_BAD == 0 && CHIMS_FIRST == 1 && IRS_BAD == 0 && IRS_FIRST == 1,
              "bad_preset and bad_count take the pair at the front of the block");
static void bad_preset(unsigned long long *small) { small[0] = 0; small[1] = ~0ull; }
static void bad_count(const unsigned long long *small, uint64_t n, uint64_t *n_bad, uint64_t *first_bad) {
    *n_bad = small[0]; *first_bad = small[0] ? small[1] : n;
}
static void bad_unpack(unsigned long long packed, uint64_t *index, uint32_t *reason) { *index = packed >> 8; *reason = (uint32_t)(packed & 0xffu); }

extern "C" {

// the characterisation stage's counting loop (include/nanosim_amd.h: ns_cs_hist; src/besthit_to_histogram.py:316-365)
struct CsSmall {                                 // what CsHistDev's dic, err and misc point into, on the device and read back
    unsigned long long dic[5][1001], error_list[18], first_error[3], spare[3], max_match, n_match2d_overflow, n_skip, spare2[5];
};
static int histograms(ns_ctx *ctx, const uint8_t *cs, const uint8_t *qry, bool maf, uint64_t nbytes, const uint64_t *aln_off, uint32_t n_aln, ns_cs_hist *h) {
    if (!ctx) return NS_EINVAL;
    if (!h || (n_aln && (!aln_off || (!cs && nbytes)))) return fail(ctx, NS_EINVAL, "ns_cs_histograms: null argument");
    if (int rc = check_offsets(ctx, "ns_cs_histograms", "strings", aln_off, n_aln, nbytes)) return rc;
    const uint32_t cap = h->cap_match2d;
    if (h->match_list && (!cap || cap > 65536u)) return fail(ctx, NS_EINVAL, "ns_cs_histograms: cap_match2d must be 1 .. 65536");
    HIPCHK(hipSetDevice(ctx->device));
    const size_t n_m2 = h->match_list ? (size_t)cap * cap : 0;
    memset(h->dic, 0, sizeof h->dic); memset(h->error_list, 0, sizeof h->error_list); memset(h->first_error, 0, sizeof h->first_error);
    h->max_match = h->n_match2d_overflow = h->n_skip = 0; h->ms_kernel = 0;
    if (!n_aln) { if (n_m2) memset(h->match_list, 0, n_m2 * 8); return NS_OK; }
    CsSmall small;
    CallScratch s(ctx, "ns_cs_histograms");
    const uint8_t *d_cs = s.filled(cs, (size_t)nbytes, NS_WINDOW_PAD), *d_qry = maf ? s.filled(qry, (size_t)nbytes, NS_WINDOW_PAD) : nullptr;
    const uint64_t *d_off = s.filled(aln_off, (size_t)n_aln + 1);
    CsSmall *d_small = s.zeroed<CsSmall>(1);
    unsigned long long *d_m2 = n_m2 ? s.zeroed<unsigned long long>(n_m2) : nullptr;
    if (int rc = s.upload()) return rc;
    if (int rc = begin(s)) return rc;
    const uint32_t *d_order = order_by_length(s, d_off, n_aln);
    const CsHistDev H{&d_small->dic[0][0], d_small->error_list, &d_small->max_match, d_m2, cap};
    per_thread(s, k_cs_hist, n_aln, d_cs, d_off, n_aln, H, d_order, d_qry);
    if (int rc = finish(s, {{&small, d_small, sizeof small}, {h->match_list, d_m2, n_m2 * 8}}, &h->ms_kernel)) return rc;
    memcpy(h->dic, small.dic, sizeof h->dic); memcpy(h->error_list, small.error_list, sizeof h->error_list); memcpy(h->first_error, small.first_error, sizeof h->first_error);
    h->max_match = small.max_match; h->n_match2d_overflow = small.n_match2d_overflow; h->n_skip = small.n_skip;
    return NS_OK;
}

int ns_cs_histograms(ns_ctx *ctx, const uint8_t *cs, uint64_t nbytes, const uint64_t *aln_off, uint32_t n_aln, ns_cs_hist *h) {
    return histograms(ctx, cs, nullptr, false, nbytes, aln_off, n_aln, h);
}
int ns_maf_histograms(ns_ctx *ctx, const uint8_t *ref_lines, const uint8_t *query_lines, uint64_t nbytes, const uint64_t *aln_off, uint32_t n_aln, ns_cs_hist *h) {
    if (ctx && n_aln && nbytes && !query_lines) return fail(ctx, NS_EINVAL, "ns_maf_histograms: null argument");
    return histograms(ctx, ref_lines, query_lines, true, nbytes, aln_off, n_aln, h);
}

// the base-quality histograms of the training side (include/nanosim_amd.h: ns_qual_hist; src/model_base_qualities.py:23-79)
int ns_qual_histograms(ns_ctx *ctx, const uint8_t *cs, uint64_t cs_bytes, const uint64_t *cs_off, const uint8_t *qual, uint64_t qual_bytes,
                       const uint64_t *qual_off, const ns_qual_aln *aln, uint32_t n_aln, ns_qual_hist *out) {
    if (!ctx) return NS_EINVAL;
    if (!out || (n_aln && (!cs_off || !qual_off || !aln || (!cs && cs_bytes) || (!qual && qual_bytes)))) return fail(ctx, NS_EINVAL, "ns_qual_histograms: null argument");
    if (int rc = check_offsets(ctx, "ns_qual_histograms", "strings", cs_off, n_aln, cs_bytes)) return rc;
    if (int rc = check_offsets(ctx, "ns_qual_histograms", "strings", qual_off, n_aln, qual_bytes)) return rc;
    for (uint32_t a = 0; a < n_aln; ++a)
        if ((uint64_t)aln[a].head + aln[a].tail > qual_off[a + 1] - qual_off[a])
            return fail(ctx, NS_EINVAL, "ns_qual_histograms: soft clips longer than the quality string of alignment " + std::to_string(a));
    memset(out, 0, sizeof *out);
    if (!n_aln) return NS_OK;
    HIPCHK(hipSetDevice(ctx->device));
    const size_t n_marks = (size_t)(qual_bytes / 16u) + 2u;               // 2 bits per quality byte, in whole words
    unsigned long long res[NS_QH_OUT_WORDS];
    CallScratch s(ctx, "ns_qual_histograms");
    const uint8_t *d_cs = s.filled(cs, (size_t)cs_bytes, NS_WINDOW_PAD);
    const uint8_t *d_qual = s.filled(qual, (size_t)qual_bytes, 32);       // (32: k_qual_count loads 16-byte words, the last of which may begin at the last byte)
    const uint64_t *d_cs_off = s.filled(cs_off, (size_t)n_aln + 1), *d_qual_off = s.filled(qual_off, (size_t)n_aln + 1);
    const ns_qual_aln *d_aln = s.filled(aln, (size_t)n_aln);
    uint32_t *d_marks = s.alloc<uint32_t>(n_marks);
    unsigned long long *d_out = s.zeroed<unsigned long long>(NS_QH_OUT_WORDS);
    if (int rc = s.upload()) return rc;
    if (int rc = begin(s)) return rc;
    s.check(hipMemsetAsync(d_marks, 0, n_marks * 4, ctx->stream));        // (inside ms_kernel: the mark phase needs it on every call)
    const uint32_t *d_order = order_by_length(s, d_cs_off, n_aln);
    per_thread(s, k_qual_mark, n_aln, d_cs, d_cs_off, d_qual_off, d_aln, n_aln, d_order, d_marks, d_out);
    // a workgroup counts a contiguous span of tiles: at most 512 workgroups (its 60 KB of counters let two of them share a compute unit:
    // one resident set, one flush each), but never more than 2^31 bytes per workgroup (32-bit counters in LDS)
    const uint64_t n_tiles = (qual_off[n_aln] + NS_QH_TILE - 1u) / NS_QH_TILE;
    const uint64_t tiles_per_wg = std::min<uint64_t>(std::max<uint64_t>((n_tiles + 511u) / 512u, 1u), (1ull << 31) / NS_QH_TILE);
    if (n_tiles && !(ctx->knob.dbg & (1u << 20)))                         // (NS_DEBUG_SKIP 1 << 20, profiling only: the mark phase alone)
        launch(s, k_qual_count, dim3((uint32_t)((n_tiles + tiles_per_wg - 1u) / tiles_per_wg)), dim3(256), d_qual, d_marks, d_qual_off, d_aln, n_aln,
                 tiles_per_wg, n_tiles, d_out);
    if (int rc = finish(s, {{res, d_out, sizeof res}}, &out->ms_kernel)) return rc;
    for (int c = 0; c < 5; ++c) for (int q = 0; q < 128; ++q) out->hist[c][q] = res[(size_t)c * 128 + q];
    out->n_short = res[NS_QH_OUT_SHORT]; out->n_bad_qual = res[NS_QH_OUT_BAD];
    return NS_OK;
}

// the homopolymer-length model of the training side (include/nanosim_amd.h: ns_hp_hist; src/model_homopolymer_lengths.py:9-119).  Two entry
// points — the lines come from the host (ns_hp_histograms) or are made on the device from SAM records (ns_hp_histograms_sam) — share
// everything from the point where the lines are on the device: HpCall holds the call's counting buffers, hp_check its arguments,
// hp_buffers asks for the memory (in front of upload()), hp_kernels runs k_hp_count (+ the scan and k_hp_records), hp_finish reads back.
struct HpCall {
    uint32_t cap_ref, cap_read; size_t n_table; uint64_t cap_records;
    unsigned long long *d_small, *d_table, *d_cnt, *d_slot; ns_hp_record *d_rec;
    unsigned long long small[HPT_WORDS];
};
static int hp_check(ns_ctx *ctx, const std::string &call, uint32_t min_hp_len, ns_hp_hist *out, HpCall &h) {
    if (!min_hp_len) return fail(ctx, NS_EINVAL, call + ": min_hp_len must be at least 1");
    h.cap_ref = out->cap_ref; h.cap_read = out->cap_read;
    if (!h.cap_ref || h.cap_ref > 65536u || !h.cap_read || h.cap_read > 65536u) return fail(ctx, NS_EINVAL, call + ": cap_ref and cap_read must be 1 .. 65536");
    if ((uint64_t)h.cap_ref * h.cap_read > (1ull << 26)) return fail(ctx, NS_EINVAL, call + ": cap_ref * cap_read must not exceed 2^26");
    h.n_table = (size_t)2 * h.cap_ref * h.cap_read;
    h.cap_records = out->records ? out->cap_records : 0;
    out->n_hp = out->max_ref = out->max_read = out->n_overflow = 0; out->ms_kernel = 0;
    memset(out->columns, 0, sizeof out->columns);
    memset(h.small, 0, sizeof h.small);
    return NS_OK;
}
static void hp_buffers(CallScratch &s, uint32_t n_aln, const ns_hp_hist *out, HpCall &h) {
    h.d_small = s.zeroed<unsigned long long>(HPT_WORDS); h.d_table = s.zeroed<unsigned long long>(h.n_table);
    h.d_cnt = s.zeroed<unsigned long long>((size_t)n_aln + 1);           // (entry n_aln stays 0: the scan leaves the total in slot[n_aln])
    h.d_slot = out->records ? s.alloc<unsigned long long>((size_t)n_aln + 1) : nullptr;
    h.d_rec = h.cap_records ? s.alloc<ns_hp_record>((size_t)h.cap_records) : nullptr;
}
// the lines are on the device (NS_WINDOW_PAD bytes to spare behind them)
static void hp_kernels(CallScratch &s, const uint8_t *d_ref, const uint8_t *d_qry, const uint64_t *d_off, uint32_t n_aln, uint32_t min_hp_len,
                       const ns_hp_hist *out, HpCall &h) {
    const uint32_t *d_order = order_by_length(s, d_off, n_aln);
    const HpTrainDev H{h.d_table, h.d_small, h.cap_ref, h.cap_read};
    per_thread(s, k_hp_count, n_aln, d_ref, d_qry, d_off, n_aln, min_hp_len, H, d_order, h.d_cnt);
    if (!out->records) return;
    scan(s, h.d_cnt, h.d_slot, (size_t)n_aln + 1);
    if (h.cap_records) per_thread(s, k_hp_records, n_aln, d_ref, d_qry, d_off, n_aln, min_hp_len, d_order, h.d_slot, h.d_rec, h.cap_records);
}
// behind finish() (which has read h.small and the table back)
static int hp_finish(CallScratch &s, ns_hp_hist *out, HpCall &h) {
    if (h.small[HPT_N_HP] && h.small[HPT_N_HP] <= h.cap_records)
        if (int rc = s.check(hipMemcpy(out->records, h.d_rec, (size_t)h.small[HPT_N_HP] * sizeof(ns_hp_record), hipMemcpyDeviceToHost))) return rc;
    for (int c = 0; c < 4; ++c) out->columns[c] = h.small[HPT_COLUMNS + c];
    out->n_hp = h.small[HPT_N_HP]; out->n_overflow = h.small[HPT_OVERFLOW]; out->max_ref = h.small[HPT_MAX_REF]; out->max_read = h.small[HPT_MAX_READ];
    return NS_OK;
}

int ns_hp_histograms(ns_ctx *ctx, const uint8_t *ref_lines, const uint8_t *query_lines, uint64_t nbytes, const uint64_t *aln_off, uint32_t n_aln,
                     uint32_t min_hp_len, ns_hp_hist *out) {
    if (!ctx) return NS_EINVAL;
    if (!out || !out->table || (n_aln && (!aln_off || ((!ref_lines || !query_lines) && nbytes)))) return fail(ctx, NS_EINVAL, "ns_hp_histograms: null argument");
    if (int rc = check_offsets(ctx, "ns_hp_histograms", "lines", aln_off, n_aln, nbytes)) return rc;
    for (uint32_t a = 0; a < n_aln; ++a)
        if (aln_off[a + 1] - aln_off[a] >= (1ull << 24))        // (the 32-bit counters of a workgroup of k_hp_count, the 30 bits of a record's read_len)
            return fail(ctx, NS_EINVAL, "ns_hp_histograms: alignment " + std::to_string(a) + " has 2^24 columns or more");
    HpCall h;
    if (int rc = hp_check(ctx, "ns_hp_histograms", min_hp_len, out, h)) return rc;
    if (!n_aln) { memset(out->table, 0, h.n_table * 8); return NS_OK; }
    HIPCHK(hipSetDevice(ctx->device));
    CallScratch s(ctx, "ns_hp_histograms");
    const uint8_t *d_ref = s.filled(ref_lines, (size_t)nbytes, NS_WINDOW_PAD), *d_qry = s.filled(query_lines, (size_t)nbytes, NS_WINDOW_PAD);
    const uint64_t *d_off = s.filled(aln_off, (size_t)n_aln + 1);
    hp_buffers(s, n_aln, out, h);
    if (int rc = s.upload()) return rc;
    if (int rc = begin(s)) return rc;
    hp_kernels(s, d_ref, d_qry, d_off, n_aln, min_hp_len, out, h);
    if (int rc = finish(s, {{h.small, h.d_small, sizeof h.small}, {out->table, h.d_table, h.n_table * 8}}, &out->ms_kernel)) return rc;
    return hp_finish(s, out, h);
}

// the line pairs of SAM records (include/nanosim_amd.h: ns_sam_pairs; ns_sam_pairs.h; src/pairwise2maf.py:38-82).  SamCall: the device side of
// the conversion for both of its callers.  Every buffer is asked for in front of upload(), the lines too: a record has at most one
// column per SEQ byte and per MD byte, so they are sized from the input and the stream never waits for the host between the phases
// (k_sam_lines reads the total from the scan's last entry).
struct SamCall {
    const uint8_t *d_cigar, *d_md, *d_seq; const uint64_t *d_cigar_off, *d_md_off, *d_seq_off;
    ns_sam_aln *d_aln; uint64_t *d_cols, *d_off; uint32_t *d_nexc; SamExc *d_exc; unsigned long long *d_small;
    uint8_t *d_ref, *d_qry; uint64_t max_bytes;
    unsigned long long small[SAMS_WORDS];
};
static int sam_check(ns_ctx *ctx, const std::string &call, const uint8_t *cigar, const uint64_t *cigar_off, const uint8_t *md, const uint64_t *md_off,
                     const uint8_t *seq, const uint64_t *seq_off, uint32_t n_aln, ns_sam_pairs *p) {
    if (n_aln && (!cigar_off || !md_off || !seq_off)) return fail(ctx, NS_EINVAL, call + ": null argument");
    if (p && (!p->aln_off || !p->ref_lines != !p->query_lines)) return fail(ctx, NS_EINVAL, call + ": null argument");
    if (!n_aln) return NS_OK;
    if (int rc = check_offsets(ctx, call.c_str(), "CIGAR strings", cigar_off, n_aln, cigar_off[n_aln])) return rc;
    if (int rc = check_offsets(ctx, call.c_str(), "MD strings", md_off, n_aln, md_off[n_aln])) return rc;
    if (int rc = check_offsets(ctx, call.c_str(), "SEQ strings", seq_off, n_aln, seq_off[n_aln])) return rc;
    if ((!cigar && cigar_off[n_aln]) || (!md && md_off[n_aln]) || (!seq && seq_off[n_aln])) return fail(ctx, NS_EINVAL, call + ": null argument");
    return NS_OK;
}
static void sam_clear(ns_sam_pairs *p, uint32_t n_aln) {
    if (!p) return;
    p->n_bytes = p->n_bad = 0; p->first_bad = n_aln; p->ms_kernel = 0;
    for (uint32_t a = 0; a <= n_aln; ++a) p->aln_off[a] = 0;
    if (p->aln && n_aln) memset(p->aln, 0, (size_t)n_aln * sizeof(ns_sam_aln));
}
static void sam_buffers(CallScratch &s, const uint8_t *cigar, const uint64_t *cigar_off, const uint8_t *md, const uint64_t *md_off, const uint8_t *seq,
                        const uint64_t *seq_off, uint32_t n_aln, bool lines, SamCall &c) {
    const size_t n = (size_t)n_aln + 1;
    c.d_cigar = s.filled(cigar, (size_t)cigar_off[n_aln], NS_WINDOW_PAD); c.d_md = s.filled(md, (size_t)md_off[n_aln], NS_WINDOW_PAD);
    c.d_seq = s.filled(seq, (size_t)seq_off[n_aln], NS_WINDOW_PAD);
    c.d_cigar_off = s.filled(cigar_off, n); c.d_md_off = s.filled(md_off, n); c.d_seq_off = s.filled(seq_off, n);
    c.d_aln = s.alloc<ns_sam_aln>(n_aln);
    c.d_cols = s.zeroed<uint64_t>(n);                                    // (entry n_aln stays 0: the scan leaves the total in d_off[n_aln])
    c.d_off = s.alloc<uint64_t>(n);
    c.d_nexc = s.alloc<uint32_t>(n_aln);
    c.d_exc = s.alloc<SamExc>((size_t)((cigar_off[n_aln] >> 1) + md_off[n_aln] + n));      // (sam_exc_base of record n_aln)
    bad_preset(c.small);
    c.d_small = s.filled(c.small, SAMS_WORDS);
    c.max_bytes = (seq_off[n_aln] - seq_off[0]) + (md_off[n_aln] - md_off[0]);
    c.d_ref = c.d_qry = nullptr;
    if (lines) {                                                         // whole 16-byte words of k_sam_lines + the window loads of k_hp_count behind them
        const size_t bytes = (size_t)((c.max_bytes + 15u) & ~(uint64_t)15u) + 16u;
        c.d_ref = s.alloc<uint8_t>(bytes); c.d_qry = s.alloc<uint8_t>(bytes);
    }
}
static void sam_kernels(CallScratch &s, uint32_t n_aln, SamCall &c) {
    per_thread(s, k_sam_scan, n_aln, c.d_cigar, c.d_cigar_off, c.d_md, c.d_md_off, c.d_seq, c.d_seq_off, n_aln, c.d_aln, c.d_cols, c.d_nexc, c.d_exc, c.d_small);
    scan(s, c.d_cols, c.d_off, (size_t)n_aln + 1);
    if (c.d_ref && c.max_bytes)
        per_thread(s, k_sam_lines, (c.max_bytes + NS_SAM_WORD - 1u) / NS_SAM_WORD, c.d_md, c.d_md_off, c.d_seq, c.d_seq_off, c.d_cigar_off, c.d_aln, c.d_nexc,
                     c.d_exc, c.d_off, n_aln, c.d_ref, c.d_qry);
}
// behind finish() (which has read c.small, the offsets and the figures back): the counters, and the lines when they fit
static int sam_finish(CallScratch &s, uint32_t n_aln, ns_sam_pairs *p, SamCall &c) {
    if (!p) return NS_OK;
    p->n_bytes = p->aln_off[n_aln];
    bad_count(c.small, n_aln, &p->n_bad, &p->first_bad);
    if (p->ref_lines && p->n_bytes && p->n_bytes <= p->cap_bytes) {
        if (int rc = s.check(hipMemcpy(p->ref_lines, c.d_ref, (size_t)p->n_bytes, hipMemcpyDeviceToHost))) return rc;
        if (int rc = s.check(hipMemcpy(p->query_lines, c.d_qry, (size_t)p->n_bytes, hipMemcpyDeviceToHost))) return rc;
    }
    return NS_OK;
}

int ns_sam_pairs_build(ns_ctx *ctx, const uint8_t *cigar, const uint64_t *cigar_off, const uint8_t *md, const uint64_t *md_off,
                       const uint8_t *seq, const uint64_t *seq_off, uint32_t n_aln, ns_sam_pairs *out) {
    if (!ctx) return NS_EINVAL;
    if (!out) return fail(ctx, NS_EINVAL, "ns_sam_pairs_build: null argument");
    if (int rc = sam_check(ctx, "ns_sam_pairs_build", cigar, cigar_off, md, md_off, seq, seq_off, n_aln, out)) return rc;
    sam_clear(out, n_aln);
    if (!n_aln) return NS_OK;
    if (seq_off[n_aln] - seq_off[0] + md_off[n_aln] - md_off[0] >= (1ull << 40)) return fail(ctx, NS_EINVAL, "ns_sam_pairs_build: more than 2^40 bytes of SEQ and MD");
    HIPCHK(hipSetDevice(ctx->device));
    SamCall c;
    CallScratch s(ctx, "ns_sam_pairs_build");
    sam_buffers(s, cigar, cigar_off, md, md_off, seq, seq_off, n_aln, out->ref_lines != nullptr, c);
    if (int rc = s.upload()) return rc;
    if (int rc = begin(s)) return rc;
    sam_kernels(s, n_aln, c);
    if (int rc = finish(s, {{c.small, c.d_small, sizeof c.small}, {out->aln_off, c.d_off, ((size_t)n_aln + 1) * 8},
                           {out->aln, c.d_aln, out->aln ? (size_t)n_aln * sizeof(ns_sam_aln) : 0}}, &out->ms_kernel)) return rc;
    return sam_finish(s, n_aln, out, c);
}
int ns_hp_histograms_sam(ns_ctx *ctx, const uint8_t *cigar, const uint64_t *cigar_off, const uint8_t *md, const uint64_t *md_off,
                         const uint8_t *seq, const uint64_t *seq_off, uint32_t n_aln, uint32_t min_hp_len, ns_sam_pairs *pairs, ns_hp_hist *out) {
    if (!ctx) return NS_EINVAL;
    if (!out || !out->table) return fail(ctx, NS_EINVAL, "ns_hp_histograms_sam: null argument");
    if (int rc = sam_check(ctx, "ns_hp_histograms_sam", cigar, cigar_off, md, md_off, seq, seq_off, n_aln, pairs)) return rc;
    HpCall h;
    if (int rc = hp_check(ctx, "ns_hp_histograms_sam", min_hp_len, out, h)) return rc;
    sam_clear(pairs, n_aln);
    memset(out->table, 0, h.n_table * 8);
    if (!n_aln) return NS_OK;
    if (seq_off[n_aln] - seq_off[0] + md_off[n_aln] - md_off[0] >= (1ull << 40)) return fail(ctx, NS_EINVAL, "ns_hp_histograms_sam: more than 2^40 bytes of SEQ and MD");
    HIPCHK(hipSetDevice(ctx->device));
    SamCall c;
    CallScratch s(ctx, "ns_hp_histograms_sam");
    sam_buffers(s, cigar, cigar_off, md, md_off, seq, seq_off, n_aln, true, c);
    hp_buffers(s, n_aln, out, h);
    if (int rc = s.upload()) return rc;
    if (int rc = begin(s)) return rc;
    sam_kernels(s, n_aln, c);
    mark(s);
    // (a bad record has no columns: the walks below are safe whatever the input was; their counts are dropped further down)
    hp_kernels(s, c.d_ref, c.d_qry, c.d_off, n_aln, min_hp_len, out, h);
    if (int rc = finish(s, {{c.small, c.d_small, sizeof c.small}, {h.small, h.d_small, sizeof h.small}, {out->table, h.d_table, h.n_table * 8},
                           {pairs ? pairs->aln_off : nullptr, c.d_off, pairs ? ((size_t)n_aln + 1) * 8 : 0},
                           {pairs ? (void *)pairs->aln : nullptr, c.d_aln, pairs && pairs->aln ? (size_t)n_aln * sizeof(ns_sam_aln) : 0}}, &out->ms_kernel)) return rc;
    if (int rc = sam_finish(s, n_aln, pairs, c)) return rc;
    if (pairs) if (int rc = ms_to_mark(s, &pairs->ms_kernel)) return rc;
    if (c.small[SAMS_BAD]) { memset(out->table, 0, h.n_table * 8); return NS_OK; }       // nothing is counted: the caller reads pairs->n_bad
    return hp_finish(s, out, h);
}

// the error-length mixtures (include/nanosim_amd.h: ns_mixfit_result; ns_mixfit.h; src/model_fitting.py:48-105): a wavefront per start
int ns_mixture_fit(ns_ctx *ctx, int kind, const double *cdf, uint32_t n_bins, const double *starts, uint32_t n_starts, int mode, ns_mixfit_result *out) {
    if (!ctx) return NS_EINVAL;
    if (!out || !out->fits || !cdf || !starts) return fail(ctx, NS_EINVAL, "ns_mixture_fit: null argument");
    if (kind != NS_MIXFIT_MISMATCH && kind != NS_MIXFIT_INDEL) return fail(ctx, NS_EINVAL, "ns_mixture_fit: unknown kind");
    if (mode != NS_MIXFIT_FIT && mode != NS_MIXFIT_EVALUATE) return fail(ctx, NS_EINVAL, "ns_mixture_fit: unknown mode");
    if (!n_bins || n_bins > MF_MAX_BINS) return fail(ctx, NS_EINVAL, "ns_mixture_fit: n_bins must be 1 .. 65536");
    if (!n_starts) return fail(ctx, NS_EINVAL, "ns_mixture_fit: no starts");
    out->ms_kernel = 0;
    HIPCHK(hipSetDevice(ctx->device));
    const bool mis = kind == NS_MIXFIT_MISMATCH;
    std::vector<double> lnf(n_bins);
    mf_lnfact_table(lnf.data(), n_bins);
    CallScratch s(ctx, "ns_mixture_fit");
    const double *d_cdf = s.filled(cdf, (size_t)n_bins), *d_lnf = s.filled(lnf.data(), (size_t)n_bins);
    const double *d_starts = s.filled(starts, (size_t)n_starts * (mis ? 3u : 4u));
    ns_mixfit_fit *d_out = s.alloc<ns_mixfit_fit>((size_t)n_starts);
    if (int rc = s.upload()) return rc;
    if (int rc = begin(s)) return rc;
    launch(s, mis ? k_mixfit<MfMis> : k_mixfit<MfIndel>, dim3((n_starts + NS_MF_WAVES - 1u) / NS_MF_WAVES), dim3(64u * NS_MF_WAVES), d_cdf, d_lnf, n_bins,
             d_starts, n_starts, mode == NS_MIXFIT_EVALUATE, d_out);
    return finish(s, {{out->fits, d_out, (size_t)n_starts * sizeof(ns_mixfit_fit)}}, &out->ms_kernel);
}

// the lengths behind the read-length models (include/nanosim_amd.h: ns_len_result; ns_read_len.h; src/head_align_tail_dist.py:134-229):
// k_len_scan, k_len_flag, the scan of the flags, k_len_reduce
int ns_read_lengths(ns_ctx *ctx, const uint8_t *cigar, const uint64_t *cigar_off, const uint8_t *reverse, const uint32_t *ref_id,
                    const uint64_t *ref_start, const uint64_t *ref_total, uint32_t n_refs, const uint64_t *read_off, uint32_t n_reads,
                    uint32_t n_aln, int mode, const uint32_t *extra_head, const uint32_t *extra_tail, ns_len_result *out) {
    if (!ctx) return NS_EINVAL;
    if (!out || !read_off || (n_reads && !out->reads) || !extra_head != !extra_tail ||
        (n_aln && (!out->segments || !cigar_off || !reverse || !ref_id || !ref_start || !ref_total)))
        return fail(ctx, NS_EINVAL, "ns_read_lengths: null argument");
    if (mode != NS_LEN_GENOME && mode != NS_LEN_TRANSCRIPTOME) return fail(ctx, NS_EINVAL, "ns_read_lengths: unknown mode");
    if (n_aln >= (1u << 31)) return fail(ctx, NS_EINVAL, "ns_read_lengths: 2^31 records or more");
    out->n_segments = out->n_bad = 0; out->first_bad = n_aln; out->ms_kernel = 0;
    for (uint32_t r = 0; r < n_reads; ++r)
        if (read_off[r] >= read_off[r + 1]) return fail(ctx, NS_EINVAL, "ns_read_lengths: read_off not ascending (a read has at least one record)");
    if (read_off[0] != 0 || read_off[n_reads] != n_aln) return fail(ctx, NS_EINVAL, "ns_read_lengths: read_off does not run from 0 to n_aln");
    if (!n_aln) return NS_OK;
    if (int rc = check_strings(ctx, "ns_read_lengths", "CIGAR strings", cigar, cigar_off, n_aln)) return rc;
    for (uint32_t a = 0; a < n_aln; ++a) {
        if (ref_id[a] >= n_refs) return fail(ctx, NS_EINVAL, "ns_read_lengths: ref_id of record " + std::to_string(a) + " is not below n_refs");
        if (ref_start[a] >= (1ull << 62)) return fail(ctx, NS_EINVAL, "ns_read_lengths: ref_start of record " + std::to_string(a) + " is out of range");
    }
    HIPCHK(hipSetDevice(ctx->device));
    std::vector<ns_len_read> preset(n_reads);
    for (uint32_t r = 0; r < n_reads; ++r) preset[r] = ns_len_read{0u, extra_head ? extra_head[r] : NS_LEN_NONE, extra_tail ? extra_tail[r] : NS_LEN_NONE, 0u};
    unsigned long long small[LENS_WORDS];
    bad_preset(small);
    uint32_t n_seg = 0;
    const size_t n = (size_t)n_aln + 1;
    CallScratch s(ctx, "ns_read_lengths");
    const auto [d_cigar, d_cigar_off] = strings(s, cigar, cigar_off[n_aln], cigar_off, n_aln);
    const uint8_t *d_reverse = s.filled(reverse, (size_t)n_aln);
    const uint32_t *d_ref_id = s.filled(ref_id, (size_t)n_aln);
    const uint64_t *d_ref_start = s.filled(ref_start, (size_t)n_aln), *d_ref_total = s.filled(ref_total, (size_t)n_refs);
    const uint64_t *d_read_off = s.filled(read_off, (size_t)n_reads + 1);
    ns_len_read *d_reads = s.filled(preset.data(), (size_t)n_reads);
    ns_len_aln *d_aln = s.alloc<ns_len_aln>(n_aln);
    uint32_t *d_rec_read = s.alloc<uint32_t>(n_aln);
    uint32_t *d_flag = s.zeroed<uint32_t>(n);                             // (entry n_aln stays 0: the scan leaves the total in d_seg[n_aln])
    uint32_t *d_seg = s.alloc<uint32_t>(n);
    unsigned long long *d_segments = s.zeroed<unsigned long long>(n_aln);
    unsigned long long *d_small = s.filled(small, LENS_WORDS);
    if (int rc = s.upload()) return rc;
    if (int rc = begin(s)) return rc;
    const uint32_t *d_order = order_by_length(s, d_cigar_off, n_aln);
    per_thread(s, k_len_scan, n_aln, d_cigar, d_cigar_off, d_reverse, d_ref_id, d_ref_start, d_ref_total, n_aln, d_order, d_aln, d_small);
    per_thread(s, k_len_flag, n_aln, d_aln, d_ref_id, d_read_off, n_reads, n_aln, mode, d_rec_read, d_flag);
    scan(s, d_flag, d_seg, n);
    per_thread(s, k_len_reduce, n_aln, d_aln, d_rec_read, d_flag, d_seg, n_aln, d_reads, d_segments);
    if (int rc = finish(s, {{small, d_small, sizeof small}, {&n_seg, d_seg + n_aln, sizeof n_seg}, {out->reads, d_reads, (size_t)n_reads * sizeof(ns_len_read)},
                           {out->aln, d_aln, out->aln ? (size_t)n_aln * sizeof(ns_len_aln) : 0}}, &out->ms_kernel)) return rc;
    out->n_segments = n_seg;
    bad_count(small, n_aln, &out->n_bad, &out->first_bad);
    return s.check(hipMemcpy(out->segments, d_segments, (size_t)n_seg * 8, hipMemcpyDeviceToHost));
}

// the split-alignment choice of chimeric reads (include/nanosim_amd.h: ns_chim_result; ns_chimeric.h; src/get_primary_sam.py:16-31,
// 273-395).  ns_cigar_spans: k_chim_scan alone
int ns_cigar_spans(ns_ctx *ctx, const uint8_t *cigar, const uint64_t *cigar_off, uint32_t n, ns_chim_ent *out, uint64_t *n_bad,
                   uint64_t *first_bad, double *ms_kernel) {
    if (!ctx) return NS_EINVAL;
    if (!n_bad || !first_bad || !ms_kernel || (n && (!cigar_off || !out))) return fail(ctx, NS_EINVAL, "ns_cigar_spans: null argument");
    if (n >= (1u << 31)) return fail(ctx, NS_EINVAL, "ns_cigar_spans: 2^31 CIGARs or more");
    *n_bad = 0; *first_bad = n; *ms_kernel = 0;
    if (!n) return NS_OK;
    if (int rc = check_strings(ctx, "ns_cigar_spans", "CIGAR strings", cigar, cigar_off, n)) return rc;
    HIPCHK(hipSetDevice(ctx->device));
    unsigned long long small[CHIMS_WORDS] = {};
    bad_preset(small);
    CallScratch s(ctx, "ns_cigar_spans");
    const auto [d_cigar, d_off] = strings(s, cigar, cigar_off[n], cigar_off, n);
    ns_chim_ent *d_ent = s.alloc<ns_chim_ent>(n);
    unsigned long long *d_small = s.filled(small, CHIMS_WORDS);
    if (int rc = s.upload()) return rc;
    if (int rc = begin(s)) return rc;
    const uint32_t *d_order = order_by_length(s, d_off, n);
    per_thread(s, k_chim_scan, n, d_cigar, d_off, n, d_order, nullptr, d_ent, d_small);
    if (int rc = finish(s, {{small, d_small, sizeof small}, {out, d_ent, (size_t)n * sizeof(ns_chim_ent)}}, ms_kernel)) return rc;
    bad_count(small, n, n_bad, first_bad);
    return NS_OK;
}

// k_chim_scan over every entry (the primary of each read in pysam's reading), then k_chim_select: one read per thread
int ns_chimeric_select(ns_ctx *ctx, const uint8_t *cigar, const uint64_t *cigar_off, const uint64_t *ent_off, uint32_t n_reads,
                       const uint32_t *ref_id, const uint64_t *ref_start, const uint32_t *nm, const uint8_t *reverse,
                       const uint64_t *ref_total, const uint32_t *species, uint32_t n_refs, uint32_t n_species, ns_chim_result *out) {
    if (!ctx) return NS_EINVAL;
    if (!out || !ent_off || (n_species && !out->species_count)) return fail(ctx, NS_EINVAL, "ns_chimeric_select: null argument");
    out->n_gaps = out->pos_strand = out->n_bad = 0; out->first_bad = 0; out->ms_kernel = out->ms_scan = 0;
    if (n_reads >= (1u << 31)) return fail(ctx, NS_EINVAL, "ns_chimeric_select: 2^31 reads or more");
    if (ent_off[0] != 0) return fail(ctx, NS_EINVAL, "ns_chimeric_select: ent_off does not begin at 0");
    for (uint32_t r = 0; r < n_reads; ++r) {
        if (ent_off[r] > ent_off[r + 1]) return fail(ctx, NS_EINVAL, "ns_chimeric_select: ent_off decreases at read " + std::to_string(r));
        if (ent_off[r] == ent_off[r + 1]) return fail(ctx, NS_EINVAL, "ns_chimeric_select: read " + std::to_string(r) + " has no entry (the first is its primary alignment)");
    }
    const uint64_t n_ent64 = ent_off[n_reads];
    if (n_ent64 >= (1ull << 31)) return fail(ctx, NS_EINVAL, "ns_chimeric_select: 2^31 entries or more");
    const uint32_t n_ent = (uint32_t)n_ent64;
    out->first_bad = n_ent;
    for (uint32_t i = 0; i < 2u * n_species; ++i) out->species_count[i] = 0;
    if (n_refs && (!ref_total || !species)) return fail(ctx, NS_EINVAL, "ns_chimeric_select: null argument");
    for (uint32_t i = 0; i < n_refs; ++i)
        if (species[i] >= n_species) return fail(ctx, NS_EINVAL, "ns_chimeric_select: species of reference " + std::to_string(i) + " is not below n_species");
    if (!n_reads) return NS_OK;
    if (!out->reads || !out->pieces || !cigar_off || !ref_id || !ref_start || !nm || !reverse) return fail(ctx, NS_EINVAL, "ns_chimeric_select: null argument");
    if (int rc = check_strings(ctx, "ns_chimeric_select", "CIGAR strings", cigar, cigar_off, n_ent)) return rc;
    for (uint32_t a = 0; a < n_ent; ++a) {
        if (ref_id[a] >= n_refs) return fail(ctx, NS_EINVAL, "ns_chimeric_select: ref_id of entry " + std::to_string(a) + " is not below n_refs");
        if (ref_start[a] >= (1ull << 62)) return fail(ctx, NS_EINVAL, "ns_chimeric_select: ref_start of entry " + std::to_string(a) + " is out of range");
    }
    HIPCHK(hipSetDevice(ctx->device));
    // the workspace of read r: (entries) * ceil(entries / 64) words from ws_off[r] on; which CIGARs are read as pysam reads them
    std::vector<uint64_t> ws_off((size_t)n_reads + 1);
    std::vector<uint8_t> pysam(n_ent, 0);
    ws_off[0] = 0;
    for (uint32_t r = 0; r < n_reads; ++r) {
        ws_off[r + 1] = ws_off[r] + chim_ws_words(ent_off[r + 1] - ent_off[r]);
        pysam[ent_off[r]] = 1;
    }
    unsigned long long small[CHIMS_WORDS] = {};
    bad_preset(small);
    CallScratch s(ctx, "ns_chimeric_select");
    const auto [d_cigar, d_cigar_off] = strings(s, cigar, cigar_off[n_ent], cigar_off, n_ent);
    const uint64_t *d_ent_off = s.filled(ent_off, (size_t)n_reads + 1), *d_ws_off = s.filled(ws_off.data(), (size_t)n_reads + 1);
    const uint8_t *d_pysam = s.filled(pysam.data(), (size_t)n_ent), *d_reverse = s.filled(reverse, (size_t)n_ent);
    const uint32_t *d_ref_id = s.filled(ref_id, (size_t)n_ent), *d_nm = s.filled(nm, (size_t)n_ent), *d_species = s.filled(species, (size_t)n_refs);
    const uint64_t *d_ref_start = s.filled(ref_start, (size_t)n_ent), *d_ref_total = s.filled(ref_total, (size_t)n_refs);
    ns_chim_ent *d_ent = s.alloc<ns_chim_ent>(n_ent);
    ns_chim_piece *d_pieces = s.zeroed<ns_chim_piece>(n_ent);
    ns_chim_read *d_reads = s.alloc<ns_chim_read>(n_reads);
    uint64_t *d_ws = s.alloc<uint64_t>((size_t)ws_off[n_reads]);                      // (k_chim_select zeroes what it opens)
    unsigned long long *d_species_count = s.zeroed<unsigned long long>((size_t)2 * n_species);
    unsigned long long *d_small = s.filled(small, CHIMS_WORDS);
    if (int rc = s.upload()) return rc;
    if (int rc = begin(s)) return rc;
    const uint32_t *d_order = order_by_length(s, d_cigar_off, n_ent);
    per_thread(s, k_chim_scan, n_ent, d_cigar, d_cigar_off, n_ent, d_order, d_pysam, d_ent, d_small);
    mark(s);
    const uint32_t *d_read_order = order_by_length(s, d_ent_off, n_reads);
    per_thread(s, k_chim_select, n_reads, d_ent, d_ent_off, n_reads, d_read_order, d_ref_id, d_ref_start, d_nm, d_reverse, d_ref_total, d_species, d_ws, d_ws_off,
                 d_pieces, d_reads, d_species_count, d_small);
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "species_count is read back as it is");
    if (int rc = finish(s, {{small, d_small, sizeof small}, {out->reads, d_reads, (size_t)n_reads * sizeof(ns_chim_read)},
                           {out->pieces, d_pieces, (size_t)n_ent * sizeof(ns_chim_piece)},
                           {out->species_count, d_species_count, (size_t)2 * n_species * 8},
                           {out->ent, d_ent, out->ent ? (size_t)n_ent * sizeof(ns_chim_ent) : 0}}, &out->ms_kernel)) return rc;
    if (int rc = ms_to_mark(s, &out->ms_scan)) return rc;
    out->n_gaps = small[CHIMS_GAPS]; out->pos_strand = small[CHIMS_POS];
    bad_count(small, n_ent, &out->n_bad, &out->first_bad);
    return NS_OK;
}

// the EM of the abundance quantification (include/nanosim_amd.h: ns_em_problem; ns_em.h; src/get_primary_sam.py:60-84, 104-127).  The
// slots are laid out here, once per call: a stable counting sort of the entries by target — the entries already stand in (item,
// position) order.  Then groups of iterations, three kernels each, and one look at the state per group.
int ns_em_quantify(ns_ctx *ctx, const ns_em_problem *p, ns_em_result *out) {
    if (!ctx) return NS_EINVAL;
    if (!p || !out) return fail(ctx, NS_EINVAL, "ns_em_quantify: null argument");
    out->n_iter = 0; out->reserved = 0; out->n_nonfinite = 0; out->ms_kernel = 0;
    const uint32_t nt = p->n_targets, nm = p->n_multi;
    if (!nt) return fail(ctx, NS_EINVAL, "ns_em_quantify: no target");
    if (!(p->total > 0.0) || !(p->total * 100.0 < 9007199254740992.0)) return fail(ctx, NS_EINVAL, "ns_em_quantify: total must be > 0 and below 2^53 / 100");
    if (!p->max_iter || p->max_iter > (1u << 20)) return fail(ctx, NS_EINVAL, "ns_em_quantify: max_iter must be 1 .. 2^20");
    if (nt >= (1u << 31) || nm >= (1u << 31)) return fail(ctx, NS_EINVAL, "ns_em_quantify: 2^31 targets or items or more");
    if (!p->unique || !out->abundance || !out->count || !out->diff_trace || (nm && (!p->multi_off || !p->target || !p->weight)))
        return fail(ctx, NS_EINVAL, "ns_em_quantify: null argument");
    for (uint32_t t = 0; t < nt; ++t)
        if (!(p->unique[t] >= 0.0 && p->unique[t] <= p->total)) return fail(ctx, NS_EINVAL, "ns_em_quantify: unique of target " + std::to_string(t) + " is not within 0 .. total");
    uint64_t n_ent = 0;
    if (nm) {
        if (p->multi_off[0] != 0) return fail(ctx, NS_EINVAL, "ns_em_quantify: multi_off does not begin at 0");
        for (uint32_t m = 0; m < nm; ++m)
            if (p->multi_off[m] >= p->multi_off[m + 1]) return fail(ctx, NS_EINVAL, "ns_em_quantify: item " + std::to_string(m) + " has no candidate, or multi_off decreases");
        n_ent = p->multi_off[nm];
        if (n_ent >= (1ull << 40)) return fail(ctx, NS_EINVAL, "ns_em_quantify: 2^40 candidates or more");
    }
    std::vector<uint64_t> tgt_off((size_t)nt + 1, 0), slot((size_t)n_ent);
    for (uint64_t e = 0; e < n_ent; ++e) {
        if (p->target[e] >= nt) return fail(ctx, NS_EINVAL, "ns_em_quantify: candidate " + std::to_string(e) + " is not below n_targets");
        ++tgt_off[p->target[e] + 1u];
    }
    for (uint32_t t = 0; t < nt; ++t) tgt_off[t + 1] += tgt_off[t];
    {
        std::vector<uint64_t> next(tgt_off.begin(), tgt_off.end() - 1);
        for (uint64_t e = 0; e < n_ent; ++e) slot[e] = next[p->target[e]]++;
    }
    const std::vector<double> a0(nt, 100.0 / (double)nt);                              // G:60 / G:104
    EmState st0{0u, 0u, 0ull, 100.0 * (double)nt};                                     // G:62 / G:106
    for (uint32_t i = 0; i < p->max_iter; ++i) out->diff_trace[i] = 0.0;
    HIPCHK(hipSetDevice(ctx->device));
    CallScratch s(ctx, "ns_em_quantify");
    const uint64_t *d_multi_off = s.filled(p->multi_off, nm ? (size_t)nm + 1 : 0), *d_slot = s.filled(slot.data(), (size_t)n_ent);
    const uint64_t *d_tgt_off = s.filled(tgt_off.data(), (size_t)nt + 1);
    const uint32_t *d_target = s.filled(p->target, (size_t)n_ent);
    const double *d_weight = s.filled(p->weight, (size_t)nm), *d_unique = s.filled(p->unique, (size_t)nt);
    double *d_a = s.filled(a0.data(), (size_t)nt);
    double *d_count = s.zeroed<double>(nt), *d_dabs = s.zeroed<double>(nt);
    double *d_contrib = s.zeroed<double>((size_t)n_ent), *d_trace = s.zeroed<double>(p->max_iter);
    EmState *d_state = s.filled(&st0, 1);
    if (int rc = s.upload()) return rc;
    if (int rc = begin(s)) return rc;
    const uint32_t group = p->group ? p->group : 1u;
    const uint32_t accum_blocks = std::min<uint32_t>((nt + NS_EM_WAVES - 1u) / NS_EM_WAVES, 8192u);
    EmState now = st0;
    while (!now.stop) {
        for (uint32_t g = 0; g < group && now.n_iter + g < p->max_iter; ++g) {
            if (nm) per_thread(s, k_em_estep, nm, d_state, d_a, d_target, d_slot, d_multi_off, d_weight, nm, d_contrib);
            launch(s, k_em_accum, dim3(accum_blocks), dim3(64u * NS_EM_WAVES), d_state, d_contrib, d_tgt_off, d_unique, p->total, nt, d_count, d_a, d_dabs);
            launch(s, k_em_stop, dim3(1), dim3(256), d_state, d_a, d_dabs, nt, p->factor, p->max_iter, d_trace);
        }
        if (int rc = fetch(s, {{&now, d_state, sizeof now}})) return rc;
    }
    if (int rc = finish(s, {{out->abundance, d_a, (size_t)nt * 8}, {out->count, d_count, (size_t)nt * 8},
                           {out->diff_trace, d_trace, (size_t)p->max_iter * 8}}, &out->ms_kernel)) return rc;
    out->n_iter = now.n_iter; out->n_nonfinite = now.n_nonfinite;
    return NS_OK;
}

// the Markov counts of the intron-retention model (include/nanosim_amd.h: ns_ir_train_result; ns_ir_train.h;
// src/model_intron_retention.py:104-176): the rows are laid out here — a prefix sum of the row words of every read's transcript —, then
// k_ir_walk, one read per thread
int ns_ir_train(ns_ctx *ctx, const uint8_t *cigar, const uint64_t *cigar_off, const uint32_t *start, const uint32_t *chrom,
                const uint32_t *trx, uint32_t n_reads, const ns_ir_introns *introns, ns_ir_train_result *out) {
    if (!ctx) return NS_EINVAL;
    if (!out || !introns) return fail(ctx, NS_EINVAL, "ns_ir_train: null argument");
    out->first[0] = out->first[1] = 0; out->states[0] = out->states[1] = out->states[2] = out->states[3] = 0;
    out->n_bad = 0; out->first_bad = n_reads; out->ms_kernel = 0;
    if (n_reads >= (1u << 31)) return fail(ctx, NS_EINVAL, "ns_ir_train: 2^31 reads or more");
    static_assert(sizeof(IrTables) == sizeof(ns_ir_introns), "ns_ir_train.h mirrors the ABI struct");
    const IrTables T{introns->n_trx, introns->n_chrom, introns->intr_off, introns->intr_chrom, introns->intr_start, introns->intr_end,
                     introns->merged_off, introns->merged_chrom, introns->merged_start, introns->merged_end};
    if (const char *why = ir_check_tables(T)) return fail(ctx, NS_EINVAL, std::string("ns_ir_train: ") + why);
    const uint64_t n_intr = T.intr_off[T.n_trx], n_merged = T.merged_off[T.n_trx], bm_words = ir_row_words(n_intr);
    if (n_intr && !out->retained) return fail(ctx, NS_EINVAL, "ns_ir_train: null argument");
    for (uint64_t w = 0; w < bm_words; ++w) out->retained[w] = 0;
    if (!n_reads) return NS_OK;
    if (!out->state || !cigar_off || !start || !chrom || !trx) return fail(ctx, NS_EINVAL, "ns_ir_train: null argument");
    if (int rc = check_strings(ctx, "ns_ir_train", "CIGAR strings", cigar, cigar_off, n_reads)) return rc;
    if (const char *why = ir_check_reads(T, chrom, trx, n_reads)) return fail(ctx, NS_EINVAL, std::string("ns_ir_train: ") + why);
    HIPCHK(hipSetDevice(ctx->device));
    std::vector<uint64_t> row_off((size_t)n_reads + 1);
    row_off[0] = 0;
    for (uint32_t r = 0; r < n_reads; ++r)
        row_off[r + 1] = row_off[r] + (trx[r] == NS_IR_NONE ? 0u : ir_row_words(T.intr_off[trx[r] + 1u] - T.intr_off[trx[r]]));
    unsigned long long small[IRS_WORDS] = {};
    bad_preset(small);
    CallScratch s(ctx, "ns_ir_train");
    const auto [d_cigar, d_cigar_off] = strings(s, cigar, cigar_off[n_reads], cigar_off, n_reads);
    const uint64_t *d_row_off = s.filled(row_off.data(), (size_t)n_reads + 1);
    const uint32_t *d_start = s.filled(start, (size_t)n_reads), *d_chrom = s.filled(chrom, (size_t)n_reads), *d_trx = s.filled(trx, (size_t)n_reads);
    IrTables D = T;                                                                    // (intr_chrom stays on the host: the walk does not read it)
    D.intr_chrom = nullptr;
    D.intr_off = s.filled(T.intr_off, (size_t)T.n_trx + 1); D.merged_off = s.filled(T.merged_off, (size_t)T.n_trx + 1);
    D.intr_start = s.filled(T.intr_start, (size_t)n_intr, 4); D.intr_end = s.filled(T.intr_end, (size_t)n_intr, 4);
    D.merged_chrom = s.filled(T.merged_chrom, (size_t)n_merged, 4); D.merged_start = s.filled(T.merged_start, (size_t)n_merged, 4);
    D.merged_end = s.filled(T.merged_end, (size_t)n_merged, 4);
    uint32_t *d_rows = s.zeroed<uint32_t>((size_t)row_off[n_reads], 4);
    uint32_t *d_bitmap = s.zeroed<uint32_t>((size_t)bm_words + 1);
    uint8_t *d_state = s.alloc<uint8_t>(n_reads);
    unsigned long long *d_small = s.filled(small, IRS_WORDS);
    if (int rc = s.upload()) return rc;
    if (int rc = begin(s)) return rc;
    const uint32_t *d_order = order_by_length(s, d_cigar_off, n_reads);
    per_thread(s, k_ir_walk, n_reads, d_cigar, d_cigar_off, d_start, d_chrom, d_trx, n_reads, d_order, D, d_rows, d_row_off, d_bitmap, d_state, d_small);
    if (int rc = finish(s, {{small, d_small, sizeof small}, {out->state, d_state, (size_t)n_reads}, {out->retained, d_bitmap, (size_t)bm_words * 4}},
                          &out->ms_kernel)) return rc;
    out->first[0] = small[IRS_COUNT + IRC_FIRST]; out->first[1] = small[IRS_COUNT + IRC_FIRST + 1];
    for (int i = 0; i < 4; ++i) out->states[i] = small[IRS_COUNT + IRC_STATES + i];
    bad_count(small, n_reads, &out->n_bad, &out->first_bad);
    return NS_OK;
}

// the best hit per read of a MAF file (include/nanosim_amd.h: ns_maf_best_result; ns_maf_best.h; src/get_besthit_maf.py:8-56).  The host
// waits twice inside the call: for the number of `s` lines, which sizes everything behind it, and for the bad-line check, so that no
// kernel ever walks the fields of a line that has none.
int ns_maf_besthit(ns_ctx *ctx, const uint8_t *text, uint64_t nbytes, const uint8_t *names, const uint64_t *names_off, uint32_t n_names,
                   ns_maf_best_result *out) {
    if (!ctx) return NS_EINVAL;
    if (!out) return fail(ctx, NS_EINVAL, "ns_maf_besthit: null argument");
    static_assert(sizeof(MafOutLines) == sizeof(ns_maf_best_lines) && sizeof(MafOutRecord) == sizeof(ns_maf_best_record) &&
                  sizeof(MafOutFigures) == sizeof(ns_maf_best_figures), "ns_maf_best.h mirrors the ABI structs");
    TrainState &keep = ctx->train;
    keep.maf_lines.clear(); keep.maf_records.clear(); keep.maf_figures.clear();
    out->lines = nullptr; out->records = nullptr; out->figures = nullptr;
    out->n_lines = out->n_pairs = out->n_kept = out->pos_strand = 0; out->first_bad_line = 0; out->first_bad_offset = ~0ull; out->ms_kernel = 0;
    if ((nbytes && !text) || (n_names && (!names_off || !out->found))) return fail(ctx, NS_EINVAL, "ns_maf_besthit: null argument");
    if (n_names) {
        if (names_off[0]) return fail(ctx, NS_EINVAL, "ns_maf_besthit: offsets not ascending / beyond the names");
        if (int rc = check_strings(ctx, "ns_maf_besthit", "names", names, names_off, n_names)) return rc;
        memset(out->found, 0, n_names);
    }
    if (!nbytes) return NS_OK;
    const uint64_t n_wg = (nbytes + MAF_LINE_SPAN - 1u) / MAF_LINE_SPAN;
    if (n_wg >= (1ull << 31)) return fail(ctx, NS_EINVAL, "ns_maf_besthit: 2^45 bytes of text or more");
    HIPCHK(hipSetDevice(ctx->device));
    unsigned long long small[MAFS_WORDS] = {~0ull, 0ull, 0ull, 0ull};
    CallScratch s(ctx, "ns_maf_besthit");
    const uint8_t *d_text = s.filled(text, (size_t)nbytes, NS_WINDOW_PAD);
    unsigned long long *d_wg_count = s.zeroed<unsigned long long>((size_t)n_wg + 1), *d_wg_base = s.alloc<unsigned long long>((size_t)n_wg + 1);
    const DevStrings d_names = n_names ? strings(s, names, names_off[n_names], names_off, n_names) : DevStrings{nullptr, nullptr};
    uint8_t *d_found = n_names ? s.alloc<uint8_t>(n_names) : nullptr;
    unsigned long long *d_small = s.filled(small, MAFS_WORDS);
    if (int rc = s.upload()) return rc;
    if (int rc = begin(s)) return rc;
    // ---- the lines ----
    launch(s, k_maf_line_count, dim3((unsigned)n_wg), dim3(256), d_text, nbytes, d_wg_count);
    scan(s, d_wg_count, d_wg_base, (size_t)n_wg + 1);
    unsigned long long n_lines = 0;
    if (int rc = fetch(s, {{&n_lines, d_wg_base + n_wg, 8}})) return rc;
    out->n_lines = out->first_bad_line = n_lines;
    if (n_lines & 1u) return fail(ctx, NS_EINVAL, "ns_maf_besthit: an odd number of `s` lines: one is without its partner");
    if (n_lines >= (1ull << 32)) return fail(ctx, NS_EINVAL, "ns_maf_besthit: 2^31 pairs or more");
    const uint32_t n_pairs = (uint32_t)(n_lines / 2u);
    out->n_pairs = n_pairs;
    uint64_t slots = 2;
    while (slots < 2ull * n_pairs) slots <<= 1;
    uint64_t *d_starts = nullptr; MafLine *d_lines = nullptr; uint32_t *d_slot_of = nullptr, *d_flag = nullptr, *d_rank = nullptr;
    MafOutLines *d_out_lines = nullptr; MafOutRecord *d_out_records = nullptr; MafOutFigures *d_out_figures = nullptr;
    MafTable T{s.alloc<uint32_t>((size_t)slots), s.zeroed<unsigned long long>((size_t)slots), slots};
    if (n_pairs) {
        d_starts = s.alloc<uint64_t>((size_t)n_lines); d_lines = s.alloc<MafLine>((size_t)n_lines);
        d_slot_of = s.alloc<uint32_t>(n_pairs); d_flag = s.zeroed<uint32_t>((size_t)n_pairs + 1); d_rank = s.alloc<uint32_t>((size_t)n_pairs + 1);
        d_out_lines = s.alloc<MafOutLines>(n_pairs); d_out_records = s.alloc<MafOutRecord>(n_pairs); d_out_figures = s.alloc<MafOutFigures>(n_pairs);
    }
    if (int rc = s.upload()) return rc;
    s.check(hipMemsetAsync(T.owner, 0xff, (size_t)slots * 4, ctx->stream));             // MAF_EMPTY
    uint32_t n_kept = 0;
    if (n_pairs) {
        launch(s, k_maf_line_write, dim3((unsigned)n_wg), dim3(256), d_text, nbytes, d_wg_base, n_lines, d_starts);
        per_thread(s, k_maf_fields, n_lines, d_text, nbytes, d_starts, n_lines, d_lines, d_small);
        if (int rc = fetch(s, {{small, d_small, 8}})) return rc;
        if (small[MAFS_FIRST_BAD] != ~0ull) {                                           // a bad line: nothing is counted
            out->first_bad_line = small[MAFS_FIRST_BAD];
            return s.check(hipMemcpy(&out->first_bad_offset, d_starts + small[MAFS_FIRST_BAD], 8, hipMemcpyDeviceToHost));
        }
        // ---- the choice, the result ----
        per_thread(s, k_maf_choose, n_pairs, d_text, d_lines, n_pairs, T, d_slot_of, d_small);
        per_thread(s, k_maf_result, n_pairs, d_text, d_lines, n_pairs, T, d_slot_of, d_flag, d_small);
        scan(s, d_flag, d_rank, (size_t)n_pairs + 1);
        per_thread(s, k_maf_emit, n_pairs, nbytes, d_starts, d_lines, n_pairs, d_flag, d_rank, d_out_lines, d_out_records, d_out_figures);
    }
    if (n_names) per_thread(s, k_maf_names, n_names, d_text, d_lines, T, d_names.bytes, d_names.off, n_names, d_found);
    if (int rc = finish(s, {{small, d_small, sizeof small}, {&n_kept, n_pairs ? d_rank + n_pairs : nullptr, n_pairs ? (size_t)4 : (size_t)0},
                           {out->found, d_found, (size_t)n_names}}, &out->ms_kernel)) return rc;
    if (small[MAFS_FULL]) return fail(ctx, NS_EHIP, "ns_maf_besthit: the name table was exhausted");
    if (n_kept != small[MAFS_ALIGNED]) return fail(ctx, NS_EHIP, "ns_maf_besthit: the kept pairs and their ranks disagree");
    if (n_kept) {
        try { keep.maf_lines.resize(n_kept); keep.maf_records.resize(n_kept); keep.maf_figures.resize(n_kept); }
        catch (const std::bad_alloc &) { return fail(ctx, NS_ENOMEM, "ns_maf_besthit: no host memory for the result"); }
        if (int rc = fetch(s, {{keep.maf_lines.data(), d_out_lines, (size_t)n_kept * sizeof(MafOutLines)},
                              {keep.maf_records.data(), d_out_records, (size_t)n_kept * sizeof(MafOutRecord)},
                              {keep.maf_figures.data(), d_out_figures, (size_t)n_kept * sizeof(MafOutFigures)}})) return rc;
    }
    out->lines = keep.maf_lines.data(); out->records = keep.maf_records.data(); out->figures = keep.maf_figures.data();
    out->n_kept = n_kept; out->pos_strand = small[MAFS_POS];
    return NS_OK;
}

// the index of a SAM text (include/nanosim_amd.h: ns_sam_index_result; ns_sam_index.h).  The host waits once inside the call, for the
// numbers of '\n' and '\t' bytes, which size everything behind them.  Whether the text ends in '\n' — the one thing the number of lines
// needs beyond the count — the host reads from its own copy.
int ns_sam_index(ns_ctx *ctx, const uint8_t *text, uint64_t nbytes, ns_sam_index_result *out) {
    if (!ctx) return NS_EINVAL;
    if (!out) return fail(ctx, NS_EINVAL, "ns_sam_index: null argument");
    static_assert(sizeof(SamRow) == sizeof(ns_sam_row) && sizeof(SamSpan) == sizeof(ns_sam_span), "ns_sam_index.h mirrors the ABI structs");
    TrainState &keep = ctx->train;
    keep.sam_rows.clear(); keep.sam_header.clear();
    out->rows = nullptr; out->header = nullptr;
    out->n_records = out->n_header = out->n_odd = out->n_cs = out->n_md = 0; out->ms_kernel = 0;
    if (nbytes && !text) return fail(ctx, NS_EINVAL, "ns_sam_index: null argument");
    if (!nbytes) return NS_OK;
    const uint64_t n_wg = (nbytes + SAM_SPAN - 1u) / SAM_SPAN;
    if (n_wg >= (1ull << 31)) return fail(ctx, NS_EINVAL, "ns_sam_index: 2^45 bytes of text or more");
    HIPCHK(hipSetDevice(ctx->device));
    unsigned long long small[SAMI_WORDS] = {0ull, 0ull, 0ull, 0ull};
    CallScratch s(ctx, "ns_sam_index");
    const uint8_t *d_text = s.filled(text, (size_t)nbytes, NS_WINDOW_PAD);
    unsigned long long *d_wg_nl = s.zeroed<unsigned long long>((size_t)n_wg + 1), *d_wg_tab = s.zeroed<unsigned long long>((size_t)n_wg + 1);
    unsigned long long *d_nl_base = s.alloc<unsigned long long>((size_t)n_wg + 1), *d_tab_base = s.alloc<unsigned long long>((size_t)n_wg + 1);
    unsigned long long *d_small = s.filled(small, SAMI_WORDS);
    if (int rc = s.upload()) return rc;
    if (int rc = begin(s)) return rc;
    // ---- the separators ----
    launch(s, k_sam_sep_count, dim3((unsigned)n_wg), dim3(256), d_text, nbytes, d_wg_nl, d_wg_tab, d_small);
    scan(s, d_wg_nl, d_nl_base, (size_t)n_wg + 1);
    scan(s, d_wg_tab, d_tab_base, (size_t)n_wg + 1);
    unsigned long long n_nl = 0, n_tabs = 0;
    if (int rc = fetch(s, {{&n_nl, d_nl_base + n_wg, 8}, {&n_tabs, d_tab_base + n_wg, 8}})) return rc;
    const uint64_t n_lines = n_nl + (text[nbytes - 1u] == '\n' ? 0u : 1u);
    if (n_lines >= (1ull << 32)) return fail(ctx, NS_EINVAL, "ns_sam_index: 2^32 lines or more");
    uint64_t *d_line_start = s.alloc<uint64_t>((size_t)n_lines + 1), *d_line_rank = s.alloc<uint64_t>((size_t)n_lines + 1);
    uint32_t *d_hdr_flag = s.zeroed<uint32_t>((size_t)n_lines + 1), *d_hdr_rank = s.alloc<uint32_t>((size_t)n_lines + 1);
    uint64_t *d_tab_pos = s.alloc<uint64_t>((size_t)n_tabs + 1);
    uint32_t *d_tab_line = s.alloc<uint32_t>((size_t)n_tabs + 1), *d_slots = s.zeroed<uint32_t>((size_t)n_lines * SAM_TAGS);
    SamRow *d_rows = s.alloc<SamRow>((size_t)n_lines);
    SamSpan *d_header = s.alloc<SamSpan>((size_t)n_lines);
    if (int rc = s.upload()) return rc;
    // ---- the lists, the tags, the rows ----
    const SamLists L{d_line_start, d_line_rank, d_tab_pos, n_lines, nbytes};
    launch(s, k_sam_sep_write, dim3((unsigned)n_wg), dim3(256), d_text, nbytes, d_nl_base, d_tab_base, n_nl, n_tabs, n_lines, d_line_start, d_line_rank,
           d_hdr_flag, d_tab_pos, d_tab_line);
    scan(s, d_hdr_flag, d_hdr_rank, (size_t)n_lines + 1);
    if (n_tabs) per_thread(s, k_sam_tags, n_tabs, d_text, L, d_tab_line, n_tabs, d_slots);
    per_thread(s, k_sam_rows, n_lines, d_text, L, d_slots, d_hdr_rank, d_rows, d_header, d_small);
    uint32_t n_header = 0;
    if (int rc = finish(s, {{small, d_small, sizeof small}, {&n_header, d_hdr_rank + n_lines, 4}}, &out->ms_kernel)) return rc;
    if (small[SAMI_LONG]) return fail(ctx, NS_EINVAL, "ns_sam_index: a line of 2^32 bytes or more");
    if (n_header > n_lines) return fail(ctx, NS_EHIP, "ns_sam_index: the header lines and their ranks disagree");
    const uint64_t n_records = n_lines - n_header;
    try { keep.sam_rows.resize(n_records); keep.sam_header.resize(n_header); }
    catch (const std::bad_alloc &) { return fail(ctx, NS_ENOMEM, "ns_sam_index: no host memory for the result"); }
    if (int rc = fetch(s, {{keep.sam_rows.data(), d_rows, (size_t)n_records * sizeof(SamRow)},
                          {keep.sam_header.data(), d_header, (size_t)n_header * sizeof(SamSpan)}})) return rc;
    out->rows = keep.sam_rows.data(); out->header = keep.sam_header.data();
    out->n_records = n_records; out->n_header = n_header;
    out->n_odd = small[SAMI_ODD]; out->n_cs = small[SAMI_CS]; out->n_md = small[SAMI_MD];
    return NS_OK;
}

// BAM records to SAM text (include/nanosim_amd.h: ns_bam_result; ns_bam.h).  The host hops the block_size chain (one 4-byte read per
// record) and waits three times inside the call: for the bad-record check and the number of floats, for the places of the floats when
// there are any (their text is the C library's), and for the size of the text, which the page-locked result is grown to.
int ns_bam_to_sam(ns_ctx *ctx, const uint8_t *bytes, uint64_t nbytes, int final, const uint8_t *ref_names, const uint64_t *ref_off, uint32_t n_ref,
                  ns_bam_result *out) {
    if (!ctx) return NS_EINVAL;
    if (!out) return fail(ctx, NS_EINVAL, "ns_bam_to_sam: null argument");
    static_assert(NS_BAM_BAD_BLOCK_SIZE == BAM_BAD_BLOCK_SIZE && NS_BAM_BAD_TAG_COUNT == BAM_BAD_TAG_COUNT && NS_BAM_BAD_TRUNCATED == BAM_BAD_TRUNCATED,
                  "ns_bam.h mirrors the ABI's reasons");
    out->text = nullptr; out->line_off = nullptr; out->n_records = out->n_text = out->consumed = 0; out->first_bad = ~0ull; out->first_bad_offset = ~0ull;
    out->bad_reason = NS_BAM_OK; out->reserved = 0; out->ms_kernel = 0;
    if ((nbytes && !bytes) || (n_ref && !ref_off)) return fail(ctx, NS_EINVAL, "ns_bam_to_sam: null argument");
    if (n_ref) {
        if (ref_off[0]) return fail(ctx, NS_EINVAL, "ns_bam_to_sam: offsets not ascending / beyond the names");
        if (int rc = check_strings(ctx, "ns_bam_to_sam", "names", ref_names, ref_off, n_ref)) return rc;
    }
    // ---- the records: the block_size chain ----
    TrainState &keep = ctx->train;
    std::vector<uint64_t> &off = keep.bam_rec_off;
    off.clear();
    uint64_t at = 0, host_bad = ~0ull;
    uint32_t host_reason = NS_BAM_OK;
    try {
        while (nbytes - at >= 4u) {
            int32_t bs;
            memcpy(&bs, bytes + at, 4);
            if (bs < 0) { host_bad = off.size(); host_reason = NS_BAM_BAD_BLOCK_SIZE; break; }
            if ((uint64_t)bs > nbytes - at - 4u) break;                                   // a partial record
            off.push_back(at);
            at += 4ull + (uint64_t)bs;
        }
        if (host_bad == ~0ull && final && at < nbytes) { host_bad = off.size(); host_reason = NS_BAM_BAD_TRUNCATED; }
        off.push_back(at);
    } catch (const std::bad_alloc &) { return fail(ctx, NS_ENOMEM, "ns_bam_to_sam: no host memory for the record offsets"); }
    const uint64_t n64 = off.size() - 1u;
    if (n64 >= (1ull << 31)) return fail(ctx, NS_EINVAL, "ns_bam_to_sam: 2^31 records or more");
    const uint32_t n = (uint32_t)n64;
    auto bad = [&](uint64_t index, uint64_t where, uint32_t reason) { out->first_bad = index; out->first_bad_offset = where; out->bad_reason = reason; return NS_OK; };
    if (!n) return host_bad != ~0ull ? bad(host_bad, at, host_reason) : NS_OK;
    HIPCHK(hipSetDevice(ctx->device));
    unsigned long long small[BAMS_WORDS] = {~0ull, 0ull, 0ull, 0ull};
    CallScratch s(ctx, "ns_bam_to_sam");
    const auto [d_bytes, d_off] = strings(s, bytes, at, off.data(), n);
    const DevStrings d_ref = n_ref ? strings(s, ref_names, ref_off[n_ref], ref_off, n_ref) : DevStrings{nullptr, nullptr};
    const BamRefs R{d_ref.bytes, d_ref.off, n_ref};
    BamRec *d_rec = s.alloc<BamRec>(n);
    unsigned long long *d_len = s.zeroed<unsigned long long>((size_t)n + 1), *d_line_off = s.alloc<unsigned long long>((size_t)n + 1);
    uint32_t *d_slices = s.zeroed<uint32_t>((size_t)n + 1), *d_slice_off = s.alloc<uint32_t>((size_t)n + 1);
    uint64_t flt_cap = 4ull * n + 1024u;
    unsigned long long *d_flt_at = s.alloc<unsigned long long>((size_t)flt_cap);
    unsigned long long *d_small = s.filled(small, BAMS_WORDS);
    if (int rc = s.upload()) return rc;
    const dim3 rec_grid((n + 3u) / 4u), wave_each(256);                                   // a wavefront per record
    if (int rc = begin(s)) return rc;
    // ---- measure ----
    launch(s, k_bam_measure, rec_grid, wave_each, d_bytes, d_off, n, R, d_rec, d_len, d_slices, d_flt_at, flt_cap, d_small);
    if (int rc = fetch(s, {{small, d_small, sizeof small}})) return rc;
    if (small[BAMS_FIRST_BAD] != ~0ull) {
        uint64_t index; uint32_t reason;
        bad_unpack(small[BAMS_FIRST_BAD], &index, &reason);
        return bad(index, off[(size_t)index], reason);
    }
    if (host_bad != ~0ull) return bad(host_bad, at, host_reason);
    const uint64_t n_float = small[BAMS_N_FLOAT];
    if (n_float >= (1ull << 32)) return fail(ctx, NS_EINVAL, "ns_bam_to_sam: 2^32 float values or more");
    if (n_float > flt_cap) {                                                              // more floats than the list held: once more, with room for all
        flt_cap = n_float;
        d_flt_at = s.alloc<unsigned long long>((size_t)flt_cap);
        if (s.rc) return s.rc;
        s.check(hipMemsetAsync(d_small + BAMS_N_FLOAT, 0, 8, ctx->stream));
        launch(s, k_bam_measure, rec_grid, wave_each, d_bytes, d_off, n, R, d_rec, d_len, d_slices, d_flt_at, flt_cap, d_small);
    }
    // ---- the floats: their places to the host, their text back ----
    const uint32_t *d_flt_first = nullptr; const uint8_t *d_slots = nullptr;
    if (n_float) {
        try {
            keep.bam_flt_at.resize((size_t)n_float); keep.bam_flt_first.assign((size_t)n + 1, 0u); keep.bam_slots.assign((size_t)n_float * BAM_FLOAT_SLOT, 0);
        } catch (const std::bad_alloc &) { return fail(ctx, NS_ENOMEM, "ns_bam_to_sam: no host memory for the floats"); }
        std::vector<uint64_t> &fa = keep.bam_flt_at;
        if (int rc = fetch(s, {{fa.data(), d_flt_at, (size_t)n_float * 8}})) return rc;
        std::sort(fa.begin(), fa.end());                                                  // the order of the records, and inside a record the order of its tags
        uint32_t r = 0;
        for (size_t k = 0; k < fa.size(); ++k) {
            if (fa[k] > at - 4u) return fail(ctx, NS_EHIP, "ns_bam_to_sam: a float outside the records");
            while (r < n && off[r + 1u] <= fa[k]) keep.bam_flt_first[++r] = (uint32_t)k;
            float f;
            memcpy(&f, bytes + fa[k], 4);
            char buf[32];
            int l = snprintf(buf, sizeof buf, "%g", (double)f);
            if (l < 0) l = 0;
            if (l > (int)BAM_FLOAT_CHARS) l = (int)BAM_FLOAT_CHARS;
            uint8_t *slot = keep.bam_slots.data() + k * BAM_FLOAT_SLOT;
            memcpy(slot, buf, (size_t)l);
            slot[BAM_FLOAT_SLOT - 1u] = (uint8_t)l;
        }
        while (r < n) keep.bam_flt_first[++r] = (uint32_t)fa.size();
        d_flt_first = s.filled(keep.bam_flt_first.data(), (size_t)n + 1);
        d_slots = s.filled(keep.bam_slots.data(), keep.bam_slots.size());
        if (int rc = s.upload()) return rc;
        per_thread(s, k_bam_float_len, n, d_flt_first, d_slots, n, d_len);
    }
    // ---- the offsets, the text ----
    scan(s, d_len, d_line_off, (size_t)n + 1);
    scan(s, d_slices, d_slice_off, (size_t)n + 1);
    unsigned long long n_text = 0;
    uint32_t n_slices = 0;
    if (int rc = fetch(s, {{&n_text, d_line_off + n, 8}, {&n_slices, d_slice_off + n, 4}})) return rc;
    if (n_slices < n || n_slices >= (1u << 31)) return fail(ctx, n_slices < n ? NS_EHIP : NS_EINVAL, "ns_bam_to_sam: 2^31 slices or more");
    uint8_t *d_text = s.alloc<uint8_t>((size_t)n_text, 16);
    if (s.rc) return s.rc;
    if (int rc = grow(ctx, keep.bam_text, (size_t)n_text + 16)) return rc;
    if (int rc = grow(ctx, keep.bam_line_off, ((size_t)n + 1) * 8)) return rc;
    launch(s, k_bam_write, dim3((n_slices + 3u) / 4u), wave_each, d_bytes, d_off, n, R, d_rec, d_line_off, d_slice_off, n_slices, d_flt_first, d_slots, d_text, d_small);
    if (int rc = finish(s, {{small, d_small, sizeof small}, {keep.bam_text.data(), d_text, (size_t)n_text},
                           {keep.bam_line_off.data(), d_line_off, ((size_t)n + 1) * 8}}, &out->ms_kernel)) return rc;
    if (small[BAMS_MISMATCH]) return fail(ctx, NS_EHIP, "ns_bam_to_sam: the two walks of a record disagree about its line");
    out->text = keep.bam_text.data(); out->line_off = keep.bam_line_off.view<uint64_t>();
    out->n_records = n; out->n_text = n_text; out->consumed = at;
    return NS_OK;
}

// cs and MD text from the reference genome (include/nanosim_amd.h: ns_calmd_result; ns_calmd.h).  The host waits once inside the call:
// for the sizes of the two texts, which their device buffers and the page-locked result are grown to.
int ns_calmd(ns_ctx *ctx, const uint8_t *cigar, const uint64_t *cigar_off, const uint8_t *seq, const uint64_t *seq_off, const uint32_t *chrom,
             const uint32_t *pos, uint32_t n, ns_calmd_result *out) {
    if (!ctx) return NS_EINVAL;
    if (!out) return fail(ctx, NS_EINVAL, "ns_calmd: null argument");
    static_assert(NS_CALMD_BAD_CIGAR == CALMD_BAD_CIGAR && NS_CALMD_BAD_SEQ_BYTE == CALMD_BAD_SEQ_BYTE && NS_CALMD_BAD_NO_COLUMN == CALMD_BAD_NO_COLUMN,
                  "ns_calmd.h mirrors the ABI's reasons");
    out->md = out->cs = nullptr; out->md_off = out->cs_off = nullptr; out->n_bad = 0; out->first_bad = ~0ull; out->bad_reason = NS_CALMD_OK;
    out->reserved = 0; out->ms_kernel = 0;
    if (!ctx->has_ref) return fail(ctx, NS_EINVAL, "ns_calmd: no reference set (ns_set_reference)");
    if (!cigar_off || !seq_off || (n && (!chrom || !pos))) return fail(ctx, NS_EINVAL, "ns_calmd: null argument");
    if (n >= (1u << 31)) return fail(ctx, NS_EINVAL, "ns_calmd: 2^31 records or more");
    if (cigar_off[0] || seq_off[0]) return fail(ctx, NS_EINVAL, "ns_calmd: offsets not ascending from 0");
    if (int rc = check_offsets(ctx, "ns_calmd", "CIGAR strings", cigar_off, n, cigar_off[n])) return rc;
    if (int rc = check_offsets(ctx, "ns_calmd", "SEQ strings", seq_off, n, seq_off[n])) return rc;
    const uint64_t cigar_bytes = cigar_off[n], seq_bytes = seq_off[n];
    if ((cigar_bytes && !cigar) || (seq_bytes && !seq)) return fail(ctx, NS_EINVAL, "ns_calmd: null argument");
    HIPCHK(hipSetDevice(ctx->device));
    TrainState &keep = ctx->train;
    if (int rc = grow(ctx, keep.calmd_md_off, ((size_t)n + 1) * 8)) return rc;
    if (int rc = grow(ctx, keep.calmd_cs_off, ((size_t)n + 1) * 8)) return rc;
    auto result = [&] {
        out->md = keep.calmd_md.data(); out->cs = keep.calmd_cs.data();
        out->md_off = keep.calmd_md_off.view<uint64_t>(); out->cs_off = keep.calmd_cs_off.view<uint64_t>();
    };
    if (!n) {
        *keep.calmd_md_off.view<uint64_t>() = 0; *keep.calmd_cs_off.view<uint64_t>() = 0;
        if (int rc = grow(ctx, keep.calmd_md, 16)) return rc;
        if (int rc = grow(ctx, keep.calmd_cs, 16)) return rc;
        result();
        return NS_OK;
    }
    unsigned long long small[CALMDS_WORDS] = {~0ull, 0ull, 0ull, 0ull};
    CallScratch s(ctx, "ns_calmd");
    const uint8_t *d_cigar = s.filled(cigar, (size_t)cigar_bytes, NS_WINDOW_PAD), *d_seq = s.filled(seq, (size_t)seq_bytes, NS_WINDOW_PAD);
    const uint64_t *d_cigar_off = s.filled(cigar_off, (size_t)n + 1), *d_seq_off = s.filled(seq_off, (size_t)n + 1);
    const uint32_t *d_chrom = s.filled(chrom, (size_t)n), *d_pos = s.filled(pos, (size_t)n);
    CalmdOp *d_ops = s.alloc<CalmdOp>((size_t)(cigar_bytes >> 1) + n + 1);
    CalmdRec *d_rec = s.alloc<CalmdRec>(n);
    unsigned long long *d_md_len = s.zeroed<unsigned long long>((size_t)n + 1), *d_cs_len = s.zeroed<unsigned long long>((size_t)n + 1);
    unsigned long long *d_md_off = s.alloc<unsigned long long>((size_t)n + 1), *d_cs_off = s.alloc<unsigned long long>((size_t)n + 1);
    unsigned long long *d_small = s.filled(small, CALMDS_WORDS);
    if (int rc = s.upload()) return rc;
    const CalmdRef G{ctx->ref.bases, ctx->ref.chrom_off, ctx->ref.nchrom};
    const dim3 grid((n + 3u) / 4u), wave_each(256);                                       // a wavefront per record
    if (int rc = begin(s)) return rc;
    launch(s, k_calmd_measure, grid, wave_each, d_cigar, d_cigar_off, d_seq, d_seq_off, d_chrom, d_pos, n, G, d_ops, d_rec, d_md_len, d_cs_len, d_small);
    scan(s, d_md_len, d_md_off, (size_t)n + 1);
    scan(s, d_cs_len, d_cs_off, (size_t)n + 1);
    unsigned long long n_md = 0, n_cs = 0;
    if (int rc = fetch(s, {{&n_md, d_md_off + n, 8}, {&n_cs, d_cs_off + n, 8}})) return rc;
    uint8_t *d_md = s.alloc<uint8_t>((size_t)n_md, 16), *d_cs = s.alloc<uint8_t>((size_t)n_cs, 16);
    if (s.rc) return s.rc;
    if (int rc = grow(ctx, keep.calmd_md, (size_t)n_md + 16)) return rc;
    if (int rc = grow(ctx, keep.calmd_cs, (size_t)n_cs + 16)) return rc;
    launch(s, k_calmd_write, grid, wave_each, d_cigar_off, d_seq, d_seq_off, d_chrom, d_pos, n, G, d_ops, d_rec, d_md_off, d_cs_off, d_md, d_cs, d_small);
    if (int rc = finish(s, {{small, d_small, sizeof small}, {keep.calmd_md.data(), d_md, (size_t)n_md}, {keep.calmd_cs.data(), d_cs, (size_t)n_cs},
                           {keep.calmd_md_off.data(), d_md_off, ((size_t)n + 1) * 8}, {keep.calmd_cs_off.data(), d_cs_off, ((size_t)n + 1) * 8}},
                          &out->ms_kernel)) return rc;
    if (small[CALMDS_MISMATCH]) return fail(ctx, NS_EHIP, "ns_calmd: the two walks of a record disagree about its texts");
    result();
    out->n_bad = small[CALMDS_N_BAD];
    if (small[CALMDS_FIRST_BAD] != ~0ull) bad_unpack(small[CALMDS_FIRST_BAD], &out->first_bad, &out->bad_reason);
    return NS_OK;
}

}  // extern "C"
