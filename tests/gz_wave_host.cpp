// Test program (CPU tests only): the block walk of nanosim_amd/csrc/ns_gz.h on the lock-step wavefront of tests/wave64_host.h, 64 lanes,
// as a stand-alone program that is built plain and under the sanitizers (tests/test_gz_wave64.py).
//
//   gz_wave_host <jobs>          every line of the file <jobs>: <input> <counts> <start> <output>
//
// The code is built from the 256 counts (64 bits each, little-endian) of the file <counts>; the bytes of <input> stand at byte <start> of a
// 16-aligned buffer of exactly their size.  Like the device, the program measures every block first (gz_member_size) and then writes every member at its
// final place in a buffer of exactly the sum (gz_member), so members begin at any alignment.  <output> gets the members; stdout one line
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

static int job(Wave64 &wave, int k_job, const char *input, const char *counts, size_t start, const char *output) {
    const std::vector<uint8_t> in = slurp(input), counted = slurp(counts);
    uint64_t hist[256] = {0};
    if (counted.size() != sizeof hist) { fprintf(stderr, "%s: not 256 counts\n", counts); return 2; }
    memcpy(hist, counted.data(), sizeof hist);
    ns_gz_code code;
    if (gz_code_build(hist, &code) || !gz_code_valid(&code)) { fprintf(stderr, "no code\n"); return 1; }
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
    uint8_t *out = static_cast<uint8_t *>(malloc(total ? total : 1));
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
    delete[] stage; delete dev; free(out); free(mem);
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: gz_wave_host <jobs>\n"); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    Wave64 wave;
    char input[4096], counts[4096], output[4096];
    unsigned long start;
    for (int k = 0; fscanf(f, "%4095s %4095s %lu %4095s", input, counts, &start, output) == 4; ++k)
        if (int rc = job(wave, k, input, counts, (size_t)start, output)) return rc;
    fclose(f);
    return 0;
}
