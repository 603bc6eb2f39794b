// chain_wave_host.hip — TEST infrastructure: chain_host.hip plus the WAVE-PER-READ event chains of nanosim_amd/csrc/ns_chain.h
// (coop_error_list, coop_unaligned_error_list, coopk_unaligned_error_list<K>) compiled for the host on the lock-step wavefront of
// tests/wave64_host.h: 64 host threads, one per lane, every cross-lane primitive of the lists (NS_WAVE_* of ns_chain.h) a rendezvous
// of the 64.  Built by tests/test_chain_wave64.py on chain_host.hip's line plus -pthread:
//   hipcc --cuda-host-only -x hip -O2 -std=c++17 -ffp-contract=off -DNS_HOST_TEST -pthread -shared -fPIC
// (host pass only: no device code, no HIP call).  Nothing of the product links or loads this file.
#include "wave64_host.h"

static thread_local Wave64Lane chw_lane{nullptr, 0};                          // the lane this host thread is
#define NS_WAVE_SCAN(v) chw_lane.incl_scan((uint32_t)(v))
#define NS_WAVE_BALLOT(p) chw_lane.ballot(p)
#define NS_WAVE_SHFL(v, src) ((int)chw_lane.shfl((uint32_t)(v), (uint32_t)(src)))
#define NS_WAVE_READLANE(v, n) ((int)chw_lane.readlane((uint32_t)(v), (uint32_t)(n)))
#define NS_WAVE_FENCE() chw_lane.fence()
#define NS_POPCLL(x) __builtin_popcountll((unsigned long long)(x))
#define NS_CLZLL(x) __builtin_clzll((unsigned long long)(x))

#include "chain_host.hip"       // chost_pack, chost_free and variants 0-4 (thread per read): the second witness, from the same build
#include <mutex>

struct ChwLaneOut { EList32 e; uint32_t n; int32_t shift; bool overflow, range; };

// variant 5: coop_error_list                       (TM: a copy of the blob's first n_words_mix words; T: the whole blob; one CoopLds for the wave)
//         6: coop_unaligned_error_list             (T: a copy of the blob's first n_words_mix words, as k_chain<true, true> has it in LDS)
//  7 .. 10: coopk_unaligned_error_list<1 .. 4>     (the same T)
//   2, 3: chain_unaligned_error_list, thread per read, as in chain_host.hip but behind shift0 (no wave)
// Every lane has its own EvSink32 (registers on the GPU) that starts at shift0 — the engine always starts at 0; the tests put the shift
// terms on their bound with it —, and all lanes store into the one array ev[0 .. cap).  Returns 0; -1 unknown variant; -2 the wave
// stopped (the lanes diverged or one did not come: the message is on stderr); -3 the 64 lanes did not end with the same EList32, n,
// shift, overflow and range, which is what "every lane stores the same value" on the GPU assumes.
static int chw_run(const ChainHost *h, int variant, int32_t m_ref, uint64_t seed, uint64_t read, uint32_t seg, uint32_t attempt, int32_t shift0,
                   ns_event *ev, uint32_t cap, ChwLaneOut &res) {
    static std::mutex one_wave;
    static Wave64 *wave = new Wave64;                      // (never destroyed: its 64 threads end with the process)
    if (variant == 2 || variant == 3) {                    // thread per read behind the same initial shift (it reads s.shift through ev_track_open)
        const Tabs TG{h->blob.data()};
        std::vector<uint64_t> lds(h->blob.begin(), h->blob.begin() + h->ct.n_words_lds);
        const ns_key key{(uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)read, (uint32_t)(read >> 32)};
        EvSink32 s;
        s.ev = ev; s.cap = cap; s.n = 0; s.shift = shift0; s.last_ins_len = 0; s.overflow = false; s.range = false; s.stg = nullptr; s.stride = 0;
        const EList32 e = chain_unaligned_error_list(variant == 2 ? Tabs{lds.data()} : TG, h->ct, m_ref, key, seg, attempt, s);
        res = ChwLaneOut{e, s.n, s.shift, s.overflow, s.range};
        return 0;
    }
    if (variant < 5 || variant > 10) return -1;
    std::lock_guard<std::mutex> lk(one_wave);
    const Tabs TG{h->blob.data()};
    std::vector<uint64_t> mix(h->blob.begin(), h->blob.begin() + h->ct.n_words_mix);       // (+ nothing: a read behind it is out of bounds)
    const Tabs TM{mix.data()};
    const ns_key key{(uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)read, (uint32_t)(read >> 32)};
    CoopLds *lds = new CoopLds;
    std::vector<ChwLaneOut> out(Wave64::LANES);
    const ChainTab &ct = h->ct;
    const bool ok = wave->run([&](uint32_t lane) {
        chw_lane = Wave64Lane{wave, lane};
        EvSink32 s;
        s.ev = ev; s.cap = cap; s.n = 0; s.shift = shift0; s.last_ins_len = 0; s.overflow = false; s.range = false; s.stg = nullptr; s.stride = 0;
        EList32 e;
        switch (variant) {
        case 5: e = coop_error_list(TM, TG, ct, m_ref, key, seg, attempt, s, *lds, lane); break;
        case 6: e = coop_unaligned_error_list(TM, ct, m_ref, key, seg, attempt, s, lane); break;
        case 7: e = coopk_unaligned_error_list<1>(TM, ct, m_ref, key, seg, attempt, s, lane); break;
        case 8: e = coopk_unaligned_error_list<2>(TM, ct, m_ref, key, seg, attempt, s, lane); break;
        case 9: e = coopk_unaligned_error_list<3>(TM, ct, m_ref, key, seg, attempt, s, lane); break;
        default: e = coopk_unaligned_error_list<4>(TM, ct, m_ref, key, seg, attempt, s, lane); break;
        }
        out[lane] = ChwLaneOut{e, s.n, s.shift, s.overflow, s.range};
    });
    delete lds;
    if (!ok) return -2;
    for (uint32_t l = 1; l < Wave64::LANES; ++l) {
        const ChwLaneOut &a = out[0], &b = out[l];
        if (a.e.l_new != b.e.l_new || a.e.middle_ref != b.e.middle_ref || a.n != b.n || a.shift != b.shift || a.overflow != b.overflow || a.range != b.range) {
            fprintf(stderr, "chain_wave_host: variant %d, lane %u ends with {%d %d %u %d %d %d}, lane 0 with {%d %d %u %d %d %d}\n", variant, l, b.e.l_new,
                    b.e.middle_ref, b.n, b.shift, (int)b.overflow, (int)b.range, a.e.l_new, a.e.middle_ref, a.n, a.shift, (int)a.overflow, (int)a.range);
            return -3;
        }
    }
    res = out[0];
    return 0;
}

extern "C" int chostw_error_list(const void *p, int variant, int32_t m_ref, uint64_t seed, uint64_t read, uint32_t seg, uint32_t attempt, int32_t shift0,
                                 ns_event *ev, uint32_t cap, int32_t *l_new, int32_t *middle_ref, uint32_t *n_ev, int32_t *shift, int *overflow, int *range) {
    ChwLaneOut r;
    const int rc = chw_run(static_cast<const ChainHost *>(p), variant, m_ref, seed, read, seg, attempt, shift0, ev, cap, r);
    if (rc) return rc;
    *l_new = r.e.l_new; *middle_ref = r.e.middle_ref; *n_ev = r.n; *shift = r.shift; *overflow = r.overflow; *range = r.range;
    return 0;
}

#ifdef CHAIN_WAVE_MAIN
// Stand-alone program for -fsanitize=address,undefined and -fsanitize=thread (tests/test_chain_wave64.py): packs a model it makes up
// itself — match columns that give 0 for half the draws (dict-key collisions, "no two 0-matches"), short run-length tables —, and runs
// the three wave-per-read lists (K = 1 .. 4) on lengths around their block and round borders, on sinks that are too small (each of
// exactly its size on the heap: a store behind it is an error) and behind initial shifts at the bounds of the field, against the
// thread-per-read lists of the same program.  Prints the number of cases; exit status 0.
#include <cstdio>
int main() {
    const uint32_t nb = 3, nseg[3] = {2, 2, 2};
    std::vector<double> fm_hi{0.25, 0.5, 1.0}, fm_vhi{3, 9, 40};
    std::vector<int64_t> lo{0, 2, 7}, hi{2, 7, 200};
    std::vector<uint32_t> off{0, 2, 4, 6};
    std::vector<double> mm_hi, mm_vhi, vlo0{0, 0, 0};
    for (uint32_t b = 0; b < nb; ++b)
        for (uint32_t s = 0; s < nseg[b]; ++s) { mm_hi.push_back(s ? 1.0 : 0.5); mm_vhi.push_back(s ? 4.0 + b : 1.0); }
    std::vector<double> cdf[3][2];
    ns_model_tables *t = new ns_model_tables();
    t->fm_nseg = 3; t->fm_hi = fm_hi.data(); t->fm_vhi = fm_vhi.data(); t->fm_vlo0 = 0;
    t->mm_nbins = nb; t->mm_bin_lo = lo.data(); t->mm_bin_hi = hi.data(); t->mm_seg_off = off.data();
    t->mm_hi = mm_hi.data(); t->mm_vhi = mm_vhi.data(); t->mm_vlo0 = vlo0.data();
    for (int s = 0; s < 7; ++s) { t->trans[s][0] = 0.3; t->trans[s][1] = 0.7; t->trans[s][2] = 0.7; }
    for (int ty = 0; ty < 3; ++ty) {
        t->mix_w[ty] = 0.5;
        for (int c = 0; c < 2; ++c) {
            const uint32_t n = 2 + 3 * ty + c;
            for (uint32_t j = 0; j < n; ++j) cdf[ty][c].push_back(j + 1 == n ? 1.0 : (j + 1.0) / n);
            t->mix_n[ty][c] = n; t->mix_cdf[ty][c] = cdf[ty][c].data();
        }
    }
    ChainHost *h = static_cast<ChainHost *>(chost_pack(t));
    if (!h || !h->whole || !ns_coop_ok(t, off[nb])) return 1;
    unsigned cases = 0;
    auto one = [&](int variant, int witness, int32_t m_ref, uint64_t read, uint32_t cap, int32_t shift0) -> int {
        std::vector<ns_event> big(4096), got(cap);
        ChwLaneOut w, g;
        EvSink32 s;
        s.ev = big.data(); s.cap = 4096; s.n = 0; s.shift = shift0; s.last_ins_len = 0; s.overflow = false; s.range = false; s.stg = nullptr; s.stride = 0;
        const ns_key key{77u, 0u, (uint32_t)read, 0u};
        const Tabs TG{h->blob.data()};
        const EList32 e = witness == 1 ? chain_error_list_g(TG, h->ct, m_ref, key, 0, 0, s) : chain_unaligned_error_list(TG, h->ct, m_ref, key, 0, 0, s);
        w = ChwLaneOut{e, s.n, s.shift, s.n > cap, s.range};
        if (chw_run(h, variant, m_ref, 77u, read, 0, 0, shift0, got.data(), cap, g)) return 2;
        if (g.e.l_new != w.e.l_new || g.e.middle_ref != w.e.middle_ref || g.n != w.n || g.shift != w.shift || g.overflow != w.overflow || g.range != w.range) return 3;
        const uint32_t kept = w.n < cap ? w.n : cap;
        if (kept && memcmp(got.data(), big.data(), sizeof(ns_event) * kept)) return 4;
        ++cases;
        return 0;
    };
    int rc = 0;
    for (uint64_t read = 0; read < 3 && !rc; ++read) {
        for (int32_t m_ref : {1, 60, 64, 70, 130, 200, 260, 400})
            for (int v = 5; v <= 10 && !rc; ++v) rc = one(v, v == 5 ? 1 : 2, m_ref, read, 1024, 0);
        for (uint32_t cap : {0u, 1u, 63u, 64u, 65u, 100u})
            for (int v = 5; v <= 10 && !rc; ++v) rc = one(v, v == 5 ? 1 : 2, 300, read, cap, 0);
        for (int32_t shift0 : {131071, 131072 - 40, -131072, -131072 + 40})
            for (int v = 6; v <= 10 && !rc; ++v) rc = one(v, 2, 150, read, 1024, shift0);
    }
    if (rc) { fprintf(stderr, "chain_wave_host: a case differs (%d) after %u\n", rc, cases); return rc; }
    printf("%u cases equal\n", cases);
    chost_free(h);
    delete t;
    return 0;
}
#endif
