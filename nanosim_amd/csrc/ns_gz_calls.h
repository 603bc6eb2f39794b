// ns_gz_calls.h — compressed output, the host calls ("BGZF output"; the code, the walk and the kernels are ns_gz.h).  Not a
// translation unit of its own: nanosim_amd.hip includes it once behind ns_train_calls.h, whose call skeleton (CallScratch, upload, begin,
// launch, scan, fetch, finish) the two encoding calls follow.
#pragma once

// the blocks of a call's ranges: first[i] = the blocks in front of range i (n_cuts entries; the last is their number)
static int gz_plan(ns_ctx *ctx, const char *call, const uint64_t *cuts, uint32_t n_cuts, uint64_t nbytes, std::vector<uint32_t> &first) {
    if (!cuts || !n_cuts) return fail(ctx, NS_EINVAL, std::string(call) + ": no cuts");
    if (cuts[n_cuts - 1] > nbytes) return fail(ctx, NS_EINVAL, std::string(call) + ": cuts beyond the bytes");
    first.assign(n_cuts, 0);
    uint64_t n_blk = 0;
    for (uint32_t i = 0; i + 1 < n_cuts; ++i) {
        if (cuts[i] > cuts[i + 1]) return fail(ctx, NS_EINVAL, std::string(call) + ": cuts not ascending");
        n_blk += (cuts[i + 1] - cuts[i] + NS_GZ_BLOCK_BYTES - 1u) / NS_GZ_BLOCK_BYTES;
        if (n_blk >= (1ull << 31)) return fail(ctx, NS_EINVAL, std::string(call) + ": 2^31 blocks or more");
        first[i + 1] = (uint32_t)n_blk;
    }
    return NS_OK;
}

// The members of d_src's ranges (device bytes, 4-byte aligned), on the call's stream: the code (counted over d_src[0 .. nbytes) when
// `code` is null), SIZE, the scan, the offsets of the ranges to the host — `dest(total)` then names the device memory of the result, or
// null after a failure it has reported itself — and EMIT.  back: what finish() copies to the host besides (its source is filled in by
// dest).  *ms: from the first kernel to the last, the host's wait for the sizes in between included.  The call has uploaded nothing yet: every buffer is asked for here, in front of the first copy.
template <typename Dest>
static int gz_encode(CallScratch &s, const uint8_t *d_src, uint64_t nbytes, const uint64_t *cuts, uint32_t n_cuts, const std::vector<uint32_t> &first,
                     const ns_gz_code *code, uint64_t *gz_off, Dest &&dest, ReadBack *back, double *ms) {
    ns_ctx *ctx = s.ctx;
    const uint32_t n_blk = first[n_cuts - 1];
    if (code && !gz_code_valid(code)) return fail(ctx, NS_EINVAL, std::string(s.call) + ": not a code of ns_gz_code_build");
    const unsigned long long *d_cuts = reinterpret_cast<const unsigned long long *>(s.filled(cuts, n_cuts));
    const uint32_t *d_first = s.filled(first.data(), n_cuts);
    unsigned long long *d_hist = code ? nullptr : s.zeroed<unsigned long long>(256);
    GzDevCode *d_code = s.alloc<GzDevCode>(1);
    unsigned long long *d_size = s.zeroed<unsigned long long>((size_t)n_blk + 1), *d_at = s.alloc<unsigned long long>((size_t)n_blk + 1);
    unsigned long long *d_off = s.alloc<unsigned long long>(n_cuts), *d_mismatch = s.zeroed<unsigned long long>(1);
    if (int rc = s.upload()) return rc;
    if (int rc = begin(s)) return rc;
    ns_gz_code counted;
    if (!code) {
        uint64_t hist[256];
        const uint64_t groups = (nbytes / 4u + 256u * 16u - 1u) / (256u * 16u);
        launch(s, k_gz_hist, dim3((unsigned)std::min<uint64_t>(std::max<uint64_t>(groups, 1), 1024)), dim3(256), d_src, nbytes, d_hist);
        if (int rc = fetch(s, {{hist, d_hist, sizeof hist}})) return rc;
        gz_code_build(hist, &counted);
        code = &counted;
    }
    GzDevCode dev;
    gz_dev_code(code, &dev);
    if (!s.rc) s.check(hipMemcpyAsync(d_code, &dev, sizeof dev, hipMemcpyHostToDevice, ctx->stream));
    const GzBlocks B{d_cuts, d_first, n_cuts - 1u, n_blk};
    const dim3 grid((n_blk + GZ_WAVES - 1u) / GZ_WAVES), block(64u * GZ_WAVES);
    launch(s, k_gz_size, grid, block, d_src, B, d_code, d_size);
    scan(s, d_size, d_at, (size_t)n_blk + 1);
    per_thread(s, k_gz_offsets, n_cuts, d_first, n_cuts, d_at, d_off);
    if (int rc = fetch(s, {{gz_off, d_off, (size_t)n_cuts * 8}})) return rc;
    uint8_t *d_dst = dest(gz_off[n_cuts - 1]);
    if (!d_dst) return s.rc ? s.rc : NS_ENOMEM;
    if (back) back->src = d_dst;
    launch(s, k_gz_emit, grid, block, d_src, B, d_code, d_at, d_dst, d_mismatch);
    unsigned long long mismatch = 0;
    if (int rc = finish(s, {{&mismatch, d_mismatch, 8}, back ? *back : ReadBack{nullptr, nullptr, 0}}, ms)) return rc;
    if (mismatch) return fail(ctx, NS_EHIP, std::string(s.call) + ": the size pass and the write pass disagree about " + std::to_string(mismatch) + " blocks");
    return NS_OK;
}

extern "C" {

int ns_gz_code_build(const uint64_t hist[256], ns_gz_code *out) { return gz_code_build(hist, out); }
uint64_t ns_gz_bound(uint64_t nbytes, uint32_t n_ranges) { return gz_bound(nbytes, n_ranges); }

// the plain image `which` of the last batch
static int gz_image(ns_ctx *ctx, const char *call, int which, const uint8_t **p, uint64_t *size) {
    if (!ctx->has_batch) return fail(ctx, NS_ESTATE, std::string(call) + ": no batch");
    if (which != NS_BUF_RECORDS && which != NS_BUF_ERRLOG) return fail(ctx, NS_EINVAL, std::string(call) + ": records or error profile only");
    const void *q;
    if (result_buf(ctx, which, &q, size)) return fail(ctx, NS_EINVAL, "unknown buffer id");
    *p = static_cast<const uint8_t *>(q);
    return NS_OK;
}

int ns_gz_histogram(ns_ctx *ctx, int which, uint64_t hist[256]) {
    if (!ctx) return NS_EINVAL;
    if (!hist) return fail(ctx, NS_EINVAL, "ns_gz_histogram: null argument");
    const uint8_t *src; uint64_t size;
    if (int rc = gz_image(ctx, "ns_gz_histogram", which, &src, &size)) return rc;
    memset(hist, 0, 256 * sizeof(uint64_t));
    if (!size) return NS_OK;
    HIPCHK(hipSetDevice(ctx->device));
    CallScratch s(ctx, "ns_gz_histogram");
    unsigned long long *d_hist = s.zeroed<unsigned long long>(256);
    if (int rc = s.upload()) return rc;
    if (int rc = begin(s)) return rc;
    const uint64_t groups = (size / 4u + 256u * 16u - 1u) / (256u * 16u);
    launch(s, k_gz_hist, dim3((unsigned)std::min<uint64_t>(std::max<uint64_t>(groups, 1), 1024)), dim3(256), src, size, d_hist);
    double ms = 0;
    return finish(s, {{hist, d_hist, 256 * sizeof(uint64_t)}}, &ms);
}

int ns_gz_bytes(ns_ctx *ctx, const uint8_t *src, uint64_t nbytes, const uint64_t *cuts, uint32_t n_cuts, const ns_gz_code *code,
                uint8_t *dst, uint64_t dst_cap, uint64_t *gz_off) {
    if (!ctx) return NS_EINVAL;
    if (!gz_off || (nbytes && !src)) return fail(ctx, NS_EINVAL, "ns_gz_bytes: null argument");
    std::vector<uint32_t> first;
    if (int rc = gz_plan(ctx, "ns_gz_bytes", cuts, n_cuts, nbytes, first)) return rc;
    memset(gz_off, 0, (size_t)n_cuts * 8);
    if (!first[n_cuts - 1]) return NS_OK;
    HIPCHK(hipSetDevice(ctx->device));
    CallScratch s(ctx, "ns_gz_bytes");
    const uint8_t *d_src = s.filled(src, (size_t)nbytes);
    ReadBack back{dst, nullptr, 0};
    double ms = 0;
    return gz_encode(s, d_src, nbytes, cuts, n_cuts, first, code, gz_off, [&](uint64_t total) -> uint8_t * {
        if (total > dst_cap || !dst) { s.rc = fail(ctx, NS_EINVAL, "ns_gz_bytes: the result has " + std::to_string(total) + " bytes, dst_cap is " + std::to_string(dst_cap)); return nullptr; }
        back.bytes = (size_t)total;
        return s.alloc<uint8_t>((size_t)total);
    }, &back, &ms);
}

int ns_gz_result(ns_ctx *ctx, int which, const uint64_t *cuts, uint32_t n_cuts, const ns_gz_code *code, uint64_t *gz_off) {
    if (!ctx) return NS_EINVAL;
    if (!gz_off) return fail(ctx, NS_EINVAL, "ns_gz_result: null argument");
    const uint8_t *src; uint64_t size;
    if (int rc = gz_image(ctx, "ns_gz_result", which, &src, &size)) return rc;
    std::vector<uint32_t> first;
    if (int rc = gz_plan(ctx, "ns_gz_result", cuts, n_cuts, size, first)) return rc;
    const int k = which == NS_BUF_ERRLOG;
    ctx->gz_bytes[k] = 0;
    memset(gz_off, 0, (size_t)n_cuts * 8);
    if (!first[n_cuts - 1]) return NS_OK;
    HIPCHK(hipSetDevice(ctx->device));
    CallScratch s(ctx, "ns_gz_result");
    double ms = 0;
    const int rc = gz_encode(s, src, size, cuts, n_cuts, first, code, gz_off, [&](uint64_t total) -> uint8_t * {
        // the slot's buffer: its last image left the device before this batch took the slot (ns_io.h)
        if (int r = ensure(ctx, ctx->gz_slot[k][ctx->slot], (size_t)total)) { s.rc = r; return nullptr; }
        return ctx->gz_slot[k][ctx->slot].data();
    }, nullptr, &ms);
    if (!rc) ctx->gz_bytes[k] = gz_off[n_cuts - 1];
    if (!rc && getenv("NS_GZ_TRACE"))            // measurement aid (scripts/bench_gzip.py): one line per call on stderr
        fprintf(stderr, "[gz] buffer %d: %llu -> %llu bytes, %u blocks, %.3f ms\n", which, (unsigned long long)size, (unsigned long long)gz_off[n_cuts - 1], first[n_cuts - 1], ms);
    return rc;
}

}  // extern "C"
