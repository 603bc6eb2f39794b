// record_rare_paths_host.hip — TEST infrastructure (tests/test_record_rare_paths.py): the rare-input helpers of the record kernels
// (iupac_members, ns_device.h; marked4 / resolve16 / resolve4, ns_materialise.h) on the DEVICE source compiled for the host:
//   hipcc --cuda-host-only -x hip -O2 -std=c++17 -ffp-contract=off -DNS_HOST_TEST -shared -fPIC
// next to literal copies of the forms they replaced (the switch, the walk over every byte of a range).  Nothing of the product links or
// loads this file.
#include <new>
#include <stdint.h>
#include "../nanosim_amd/csrc/ns_materialise.h"

// ---- what the helpers replaced, kept here word for word as the reference ---------------------------------------------------------
static uint32_t members_switch(uint32_t c, uint32_t &n) {
    switch (c) {
        case 'Y': n = 2; return 'C' | 'T' << 8;
        case 'R': n = 2; return 'A' | 'G' << 8;
        case 'W': n = 2; return 'A' | 'T' << 8;
        case 'S': n = 2; return 'G' | 'C' << 8;
        case 'K': n = 2; return 'T' | 'G' << 8;
        case 'M': n = 2; return 'C' | 'A' << 8;
        case 'D': n = 3; return 'A' | 'G' << 8 | 'T' << 16;
        case 'V': n = 3; return 'A' | 'C' << 8 | 'G' << 16;
        case 'H': n = 3; return 'A' | 'C' << 8 | 'T' << 16;
        case 'B': n = 3; return 'C' | 'G' << 8 | 'T' << 16;
        case 'N': case 'X': n = 4; return 0x47435441u;
        default: n = 0; return 0;
    }
}
static uint8_t resolve_base_switch(uint32_t c, const ns_key &key, uint32_t seg, uint32_t attempt, uint32_t x) {
    if (!(c & 0x80u)) return (uint8_t)c;
    c &= 0x7fu;
    uint32_t n, mem = members_switch(c, n);
    if (!n) return (uint8_t)c;
    u32x4 w = ns_draw(key, ST_IUPAC, seg, attempt, x >> 2, 0);
    uint32_t j = (uint32_t)(((uint64_t)ns_word(w, x & 3) * n) >> 32);
    return (uint8_t)(mem >> (8 * j));
}
static void resolve16_walk(uint32_t &a0, uint32_t &a1, uint32_t &a2, uint32_t &a3, uint32_t i0, uint32_t i1, uint32_t x0,
                           const ns_key &key, uint32_t sid, uint32_t a) {
    for (uint32_t b = i0; b < i1; ++b) {
        uint32_t wk = b < 8 ? (b < 4 ? a0 : a1) : (b < 12 ? a2 : a3);
        const uint32_t ch = (wk >> (8 * (b & 3))) & 0xff;
        if (!(ch & 0x80u)) continue;
        const uint32_t r = resolve_base_switch(ch, key, sid, a, x0 + b);
        wk = (wk & ~(0xffu << (8 * (b & 3)))) | r << (8 * (b & 3));
        if (b < 4) a0 = wk; else if (b < 8) a1 = wk; else if (b < 12) a2 = wk; else a3 = wk;
    }
}

static ns_key make_key(uint64_t seed, uint64_t read) { return ns_key{(uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)read, (uint32_t)(read >> 32)}; }

extern "C" {

// out[2 c] = members, out[2 c + 1] = count, for c = 0 .. n - 1; which: 0 = the engine's iupac_members, 1 = the switch
void rr_members(uint32_t n, int which, uint32_t *out) {
    for (uint32_t c = 0; c < n; ++c) { uint32_t k = 0xdeadu; out[2 * c] = which ? members_switch(c, k) : iupac_members(c, k); out[2 * c + 1] = k; }
}
// normalise_base and resolve_base (the engine's) of every byte value at segment position x: out[c] = normalised, out[256 + c] = resolved,
// out[512 + c] = resolved by the switch form
void rr_bytes(uint64_t seed, uint64_t read, uint32_t sid, uint32_t a, uint32_t x, uint8_t *out) {
    const ns_key key = make_key(seed, read);
    for (uint32_t c = 0; c < 256; ++c) {
        out[c] = normalise_base(c);
        out[256 + c] = resolve_base(c, key, sid, a, x);
        out[512 + c] = resolve_base_switch(c, key, sid, a, x);
    }
}
uint32_t rr_marked4(uint32_t w) { return marked4(w); }

// n groups of 16 bytes (g, in place), their ranges [i0, i1) and segment positions x0.  which 0: the way the tile sites call resolve16 —
// the group masked to its range (mask16: bytes outside zeroed first, as and_andn with the mlut rows does), among = all; which 1: the way
// dense_piece calls it — the group unmasked, i0 = 0, among = the low i1 bits; which 2: the walk over every byte of [i0, i1) on the masked
// group.  Bytes outside the range come back zero for 0 and 2, untouched for 1.
void rr_resolve16(uint32_t n, int which, uint8_t *g, const uint32_t *i0, const uint32_t *i1, const uint32_t *x0, uint64_t seed, uint64_t read,
                  uint32_t sid, uint32_t a) {
    const ns_key key = make_key(seed, read);
    for (uint32_t k = 0; k < n; ++k) {
        uint32_t w[4];
        __builtin_memcpy(w, g + 16 * k, 16);
        if (which != 1)
            for (uint32_t b = 0; b < 16; ++b)
                if (b < i0[k] || b >= i1[k]) w[b >> 2] &= ~(0xffu << (8 * (b & 3)));
        if (which == 0) resolve16(w[0], w[1], w[2], w[3], 0xffffu, x0[k], key, sid, a);
        else if (which == 1) { if (i1[k]) resolve16(w[0], w[1], w[2], w[3], 0xffffu >> (16u - i1[k]), x0[k], key, sid, a); }
        else resolve16_walk(w[0], w[1], w[2], w[3], i0[k], i1[k], x0[k], key, sid, a);
        __builtin_memcpy(g + 16 * k, w, 16);
    }
}
// n dwords of four bases under a group of substitution letters of which cnt[k] (1 .. 4) are kept: which 0 = resolve4 as dense_piece
// calls it, which 1 = resolve_base (switch form) of each of the first cnt bytes
void rr_resolve4(uint32_t n, int which, uint32_t *w, const uint32_t *cnt, const uint32_t *x0, uint64_t seed, uint64_t read, uint32_t sid, uint32_t a) {
    const ns_key key = make_key(seed, read);
    for (uint32_t k = 0; k < n; ++k) {
        if (which == 0) resolve4(w[k], 0xfu >> (4u - cnt[k]), x0[k], key, sid, a);
        else
            for (uint32_t t = 0; t < cnt[k]; ++t)
                w[k] = (w[k] & ~(0xffu << (8 * t))) | (uint32_t)resolve_base_switch((w[k] >> (8 * t)) & 0xffu, key, sid, a, x0[k] + t) << (8 * t);
    }
}

}  // extern "C"
