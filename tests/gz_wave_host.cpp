// Test program (CPU tests only): the block walk of nanosim_amd/csrc/ns_gz.h on the lock-step wavefront of tests/wave64_host.h, 64 lanes,
// as a stand-alone program that is built plain and under the sanitizers (tests/test_gz_wave64.py).
//
//   gz_wave_host <jobs>          every line of the file <jobs>: <input> <counts> <start> <output> <dst start>
//   gz_wave_host code <hists>    the code builder alone, for every 256 counts of the file <hists>: "hist k rc valid header_bits", then the lines
//                                "len", "code" (257 numbers each) and "header" (the NS_GZ_HEADER_BYTES bytes in hex); at the end "null" with what
//                                gz_code_build answers to a null histogram and to a null code, and the tables of gz_dev_code, "crc_tab" (256 numbers) and "lane_pow" (64)
//   gz_wave_host valid <codes>   gz_code_valid's verdict on every ns_gz_code of the file <codes> (the bytes of the struct), one per line
//   gz_wave_host badsize <jobs>  <input> <counts> <start> per line, one block each: gz_member with the measured size + 1 and - 1 into a
//                                buffer full of a canary; "k_job size returned_plus returned_minus touched" per line
//   gz_wave_host blocks <cuts>   gz_block_at for every block of the ranges of <cuts> (64 bits each, little-endian): "g off n" per line
//
// The code is built from the 256 counts (64 bits each, little-endian) of the file <counts> - or, when the file has the size of an ns_gz_code,
// is that code as it stands, if gz_code_valid accepts it; the bytes of <input> stand at byte <start> of a
// 16-aligned buffer of exactly their size.  Like the device, the program measures every block first (gz_member_size) and then writes every member at its
// final place, from byte <dst start> of a buffer that ends with the last member (gz_member), so members begin at any alignment.  <output> gets the members; stdout one line
// per block: the job, its input bytes, its member's bytes, 1 when it is a stored block.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../nanosim_amd/csrc/ns_gz.h"
#include "wave64_host.h"

static std::vector<uint8_t> slurp(const char *path) {
    std::vector<uint8_t> v;
    FILE *f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    uint8_t buf[65536];
    for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}

// the code of the file <counts>: built from 256 counts, or an ns_gz_code as it stands
static int code_of(const char *counts, ns_gz_code *code) {
    const std::vector<uint8_t> counted = slurp(counts);
    uint64_t hist[256] = {0};
    if (counted.size() == sizeof *code) memcpy(code, counted.data(), sizeof *code);
    else if (counted.size() != sizeof hist) { fprintf(stderr, "%s: neither 256 counts nor a code\n", counts); return 2; }
    else { memcpy(hist, counted.data(), sizeof hist); if (gz_code_build(hist, code)) { fprintf(stderr, "no code\n"); return 1; } }
    if (!gz_code_valid(code)) { fprintf(stderr, "%s: no valid code\n", counts); return 1; }
    return 0;
}

static int job(Wave64 &wave, int k_job, const char *input, const char *counts, size_t start, const char *output, size_t dst_start) {
    const std::vector<uint8_t> in = slurp(input);
    ns_gz_code code;
    if (int rc = code_of(counts, &code)) return rc;
    GzDevCode *dev = new GzDevCode;
    gz_dev_code(&code, dev);
    const GzTabs T{dev->sym, dev->crc_tab, dev->header, dev->lane_pow, dev->header_bits};
    void *mem = nullptr;
    if (posix_memalign(&mem, 16, start + in.size() ? start + in.size() : 1)) return 2;
    uint8_t *src = static_cast<uint8_t *>(mem) + start;
    if (!in.empty()) memcpy(src, in.data(), in.size());

    std::vector<uint32_t> size;
    for (size_t at = 0; at < in.size(); at += NS_GZ_BLOCK_BYTES) {
        const uint32_t n = (uint32_t)(in.size() - at < NS_GZ_BLOCK_BYTES ? in.size() - at : NS_GZ_BLOCK_BYTES);
        uint32_t m = 0;
        if (!wave.run([&](uint32_t lane) { Wave64Lane w{&wave, lane}; const uint32_t v = gz_member_size(w, T, src + at, n); if (!lane) m = v; })) return 1;
        size.push_back(m);
    }
    size_t total = 0;
    for (uint32_t m : size) total += m;
    uint8_t *room = static_cast<uint8_t *>(malloc(dst_start + total ? dst_start + total : 1)), *out = room + dst_start;
    uint32_t *stage = new uint32_t[GZ_STAGE_WORDS];
    size_t o = 0;
    for (size_t k = 0; k < size.size(); ++k) {
        const size_t at = k * NS_GZ_BLOCK_BYTES;
        const uint32_t n = (uint32_t)(in.size() - at < NS_GZ_BLOCK_BYTES ? in.size() - at : NS_GZ_BLOCK_BYTES);
        uint32_t m = 0;
        if (!wave.run([&](uint32_t lane) { Wave64Lane w{&wave, lane}; const uint32_t v = gz_member(w, T, src + at, n, stage, out + o, size[k]); if (!lane) m = v; })) return 1;
        if (m != size[k]) { fprintf(stderr, "job %d block %zu: measured %u bytes, wrote %u\n", k_job, k, size[k], m); return 1; }
        printf("%d %u %u %d\n", k_job, n, m, out[o + 18] == 1 ? 1 : 0);
        o += m;
    }
    FILE *f = fopen(output, "wb");
    if (!f || fwrite(out, 1, total, f) != total || fclose(f)) { fprintf(stderr, "cannot write %s\n", output); return 2; }
    delete[] stage; delete dev; free(room); free(mem);
    return 0;
}

static int code_mode(const char *path) {
    const std::vector<uint8_t> all = slurp(path);
    if (all.size() % 2048u) { fprintf(stderr, "%s: not a multiple of 256 counts\n", path); return 2; }
    ns_gz_code code;
    for (size_t k = 0; k < all.size() / 2048u; ++k) {
        uint64_t hist[256];
        memcpy(hist, all.data() + 2048u * k, sizeof hist);
        const int rc = gz_code_build(hist, &code);
        printf("hist %zu %d %d %u\nlen", k, rc, gz_code_valid(&code) ? 1 : 0, code.header_bits);
        for (uint32_t v = 0; v < 257; ++v) printf(" %u", code.len[v]);
        printf("\ncode");
        for (uint32_t v = 0; v < 257; ++v) printf(" %u", code.code[v]);
        printf("\nheader ");
        for (uint32_t i = 0; i < NS_GZ_HEADER_BYTES; ++i) printf("%02x", code.header[i]);
        printf("\n");
    }
    uint64_t none[256] = {0};
    printf("null %d %d\n", gz_code_build(nullptr, &code), gz_code_build(none, nullptr));      // NS_EINVAL twice, nothing touched
    memset(&code, 0, sizeof code);
    GzDevCode *dev = new GzDevCode;
    gz_dev_code(&code, dev);
    printf("crc_tab");
    for (uint32_t v = 0; v < 256; ++v) printf(" %u", dev->crc_tab[v]);
    printf("\nlane_pow");
    for (uint32_t l = 0; l < GZ_LANES; ++l) printf(" %u", dev->lane_pow[l]);
    printf("\n");
    delete dev;
    return 0;
}

static int valid_mode(const char *path) {
    const std::vector<uint8_t> all = slurp(path);
    if (all.size() % sizeof(ns_gz_code)) { fprintf(stderr, "%s: not a multiple of a code\n", path); return 2; }
    for (size_t k = 0; k < all.size() / sizeof(ns_gz_code); ++k) {
        ns_gz_code code;
        memcpy(&code, all.data() + k * sizeof code, sizeof code);
        printf("%d\n", gz_code_valid(&code) ? 1 : 0);
    }
    return 0;
}

// gz_member with a size that is not the member's: it says the true size and stores nothing.  The member's place is the middle of a buffer
// of three times the largest member, every byte a canary
static int badsize(Wave64 &wave, int k_job, const char *input, const char *counts, size_t start) {
    const std::vector<uint8_t> in = slurp(input);
    if (in.empty() || in.size() > NS_GZ_BLOCK_BYTES) { fprintf(stderr, "%s: one block\n", input); return 2; }
    ns_gz_code code;
    if (int rc = code_of(counts, &code)) return rc;
    GzDevCode *dev = new GzDevCode;
    gz_dev_code(&code, dev);
    const GzTabs T{dev->sym, dev->crc_tab, dev->header, dev->lane_pow, dev->header_bits};
    void *mem = nullptr;
    if (posix_memalign(&mem, 16, start + in.size())) return 2;
    uint8_t *src = static_cast<uint8_t *>(mem) + start;
    memcpy(src, in.data(), in.size());
    const uint32_t n = (uint32_t)in.size(), room = 4u * GZ_STAGE_WORDS;
    uint32_t size = 0, got[2] = {0, 0};
    if (!wave.run([&](uint32_t lane) { Wave64Lane w{&wave, lane}; const uint32_t v = gz_member_size(w, T, src, n); if (!lane) size = v; })) return 1;
    std::vector<uint8_t> out(3u * room, 0xa5);
    uint32_t *stage = new uint32_t[GZ_STAGE_WORDS];
    for (int k = 0; k < 2; ++k) {
        const uint32_t expect = k ? size - 1u : size + 1u;
        uint8_t *dst = out.data() + room + (size_t)(k_job & 3);
        if (!wave.run([&](uint32_t lane) { Wave64Lane w{&wave, lane}; const uint32_t v = gz_member(w, T, src, n, stage, dst, expect); if (!lane) got[k] = v; })) return 1;
    }
    size_t touched = 0;
    for (uint8_t b : out) touched += b != 0xa5;
    printf("%d %u %u %u %zu\n", k_job, size, got[0], got[1], touched);
    delete[] stage; delete dev; free(mem);
    return 0;
}

static int blocks_mode(const char *path) {
    const std::vector<uint8_t> all = slurp(path);
    if (all.size() % 8u || all.size() < 16u) { fprintf(stderr, "%s: two cuts or more\n", path); return 2; }
    const uint32_t n_cuts = (uint32_t)(all.size() / 8u);
    std::vector<unsigned long long> cuts(n_cuts);
    memcpy(cuts.data(), all.data(), all.size());
    std::vector<uint32_t> first(n_cuts, 0u);                         // (gz_plan of ns_gz_calls.h)
    for (uint32_t i = 0; i + 1 < n_cuts; ++i) first[i + 1] = first[i] + (uint32_t)((cuts[i + 1] - cuts[i] + NS_GZ_BLOCK_BYTES - 1u) / NS_GZ_BLOCK_BYTES);
    const GzBlocks B{cuts.data(), first.data(), n_cuts - 1u, first[n_cuts - 1]};
    for (uint32_t g = 0; g < B.n_blk; ++g) {
        uint64_t off; uint32_t n;
        gz_block_at(B, g, off, n);
        printf("%u %llu %u\n", g, (unsigned long long)off, n);
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 3 && !strcmp(argv[1], "code")) return code_mode(argv[2]);
    if (argc == 3 && !strcmp(argv[1], "valid")) return valid_mode(argv[2]);
    if (argc == 3 && !strcmp(argv[1], "blocks")) return blocks_mode(argv[2]);
    if (argc == 3 && !strcmp(argv[1], "badsize")) {
        FILE *f = fopen(argv[2], "r");
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
        Wave64 wave;
        char input[4096], counts[4096];
        unsigned long start;
        for (int k = 0; fscanf(f, "%4095s %4095s %lu", input, counts, &start) == 3; ++k)
            if (int rc = badsize(wave, k, input, counts, (size_t)start)) return rc;
        fclose(f);
        return 0;
    }
    if (argc != 2) { fprintf(stderr, "usage: gz_wave_host <jobs> | code <hists> | valid <codes> | badsize <jobs> | blocks <cuts>\n"); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    Wave64 wave;
    char input[4096], counts[4096], output[4096];
    unsigned long start, dst_start;
    for (int k = 0; fscanf(f, "%4095s %4095s %lu %4095s %lu", input, counts, &start, output, &dst_start) == 5; ++k)
        if (int rc = job(wave, k, input, counts, (size_t)start, output, (size_t)dst_start)) return rc;
    fclose(f);
    return 0;
}
