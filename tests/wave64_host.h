// Test shim (CPU tests only): a wavefront of 64 lanes in LOCK STEP on the host, for the walks that are written against an abstract
// wavefront W (nanosim_amd/csrc/ns_calmd.h, ns_bam.h).  Plain C++17 with threads, no HIP and no GPU: 64 host threads, one per lane, kept
// for the life of the Wave64 object; run() hands all of them one body and returns when every lane has left it.
//
// Every collective — ballot, scan (32 and 64 bits; incl_scan is scan + the lane's own value), first, bcast, shfl, readlane, fence, and the
// two meetings of float_reserve — is a RENDEZVOUS: each
// lane deposits its value, all 64 meet, each reads the deposits.  A deposit is two atomic words, each of which names its round and the
// kind of the collective next to 32 bits of the value: a reader waits on a word until it names the round it is in, so a word is its
// own proof of being the right one and nothing else has to be ordered.  The words are kept twice and used in turn: a lane can stand at
// most one collective ahead of the slowest reader (it waits there for that reader's deposit), and that collective uses the other set.
//
// WHAT ORDERS MEMORY.  On the GPU a ballot, a prefix sum or a broadcast moves registers; it is no memory fence.  So here the deposits
// of ballot, scan, first, bcast, shfl and readlane are RELAXED atomics: a lane learns the other lanes' values from them and nothing about what those
// lanes wrote to plain memory.  Only fence() deposits with release and reads with acquire (and so do the two meetings of float_reserve,
// which stand in for an atomic add on a list the shim itself reallocates, and the hand-over of a body in run()).  Under
// -fsanitize=thread a table that one lane writes and another reads with no fence() between the two — whatever other collectives lie
// between — is therefore a data race, and so are two lanes that store to one byte.  (-DWAVE64_FENCE_ORDERS_NOTHING makes fence() a
// relaxed rendezvous like the others: what a walk looks like to the sanitizer when its fence is missing; tests/test_calmd_wave64.py
// asks that the run is refused then.)
//
// On the GPU a collective that only some lanes reach gives a partial mask, silently.  Here the wave STOPS WITH A MESSAGE, and run()
// returns false, when
//   - lanes stand at different kinds of collective in the same round,
//   - a lane waits at a collective for a lane that has left the walk,
//   - a lane waits longer than WAVE64_TIMEOUT_MS for another (a lane that loops without a collective).
// The lanes that can still be stopped leave their body through an exception at their next collective.  A lane that does not come back
// WAVE64_TIMEOUT_MS after that cannot be ended from outside: the process aborts with the message.  So does a body that no lane has
// left or stopped after WAVE64_RUN_MS (every lane loops without a collective).
#pragma once
#include <sched.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#ifndef WAVE64_TIMEOUT_MS
#define WAVE64_TIMEOUT_MS 8000
#endif
#ifndef WAVE64_RUN_MS
#define WAVE64_RUN_MS 300000                                          // one body: the walk of one record
#endif

class Wave64 {
public:
    static constexpr uint32_t LANES = 64u;
    enum Kind : uint32_t { BALLOT = 0, SCAN32, SCAN64, FIRST, BCAST, FENCE, RESERVE_IN, RESERVE_OUT, SHFL, READLANE, N_KINDS };
    struct Stop {};                                                  // what a lane leaves a stopped wave with

    Wave64() {}
    Wave64(const Wave64 &) = delete;
    Wave64 &operator=(const Wave64 &) = delete;
    ~Wave64() {
        {
            std::lock_guard<std::mutex> lk(mu_);
            quit_ = true;
        }
        cv_.notify_all();
        for (std::thread &t : threads_) t.join();
    }

    // body(lane) on all 64 lanes; true when every lane has left it and the wave was not stopped
    bool run(const std::function<void(uint32_t)> &body) {
        std::unique_lock<std::mutex> lk(mu_);
        if (threads_.empty()) for (uint32_t l = 0; l < LANES; ++l) threads_.emplace_back(&Wave64::lane_main, this, l);
        body_ = &body; error_.clear();
        done_.store(0); failed_.store(false);
        for (uint32_t l = 0; l < LANES; ++l) {                       // (a stopped body leaves its lanes in different rounds)
            round_[l] = 0;
            left_[l].store(false);
            for (Slot *set : {slots_[0], slots_[1]}) { set[l].lo.store(0, std::memory_order_relaxed); set[l].hi.store(0, std::memory_order_relaxed); }
        }
        ++job_;
        cv_.notify_all();
        // (waits on the system clock: pthread_cond_timedwait, which every -fsanitize=thread runtime knows as an unlock and a lock)
        const auto tick = std::chrono::milliseconds(50), limit = std::chrono::milliseconds(WAVE64_TIMEOUT_MS);
        const auto t0 = std::chrono::steady_clock::now();
        while (done_.load() != LANES && !failed_.load()) {
            main_cv_.wait_until(lk, std::chrono::system_clock::now() + tick);
            if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(WAVE64_RUN_MS)) {
                fprintf(stderr, "wave64: %u lanes are still in their body after %d ms and none waits at a collective, aborting\n", LANES - done_.load(), (int)WAVE64_RUN_MS);
                abort();
            }
        }
        if (!main_cv_.wait_until(lk, std::chrono::system_clock::now() + limit, [&] { return done_.load() == LANES; })) {
            fprintf(stderr, "wave64: %s; %u lanes did not come back, aborting\n", error_.c_str(), LANES - done_.load());
            abort();
        }
        body_ = nullptr;
        if (failed_.load()) fprintf(stderr, "wave64: %s\n", error_.c_str());
        return !failed_.load();
    }
    const std::string &error() const { return error_; }

    // the rendezvous: deposit v, meet the 63 others at a collective of the same kind, their deposits to got[0 .. 64)
    void meet(uint32_t lane, Kind kind, uint64_t v, uint64_t *got) {
        if (failed_.load()) throw Stop();
#ifdef WAVE64_FENCE_ORDERS_NOTHING
        const bool orders = kind == RESERVE_IN || kind == RESERVE_OUT;
#else
        const bool orders = kind == FENCE || kind == RESERVE_IN || kind == RESERVE_OUT;
#endif
        const std::memory_order put = orders ? std::memory_order_release : std::memory_order_relaxed,
                                get = orders ? std::memory_order_acquire : std::memory_order_relaxed;
        const uint32_t r = ++round_[lane];                           // (my own count: every lane is in the same round, or stands one ahead)
        const uint64_t tag = ((uint64_t)(r & 0xffffffu) << 40) | ((uint64_t)kind << 32);
        Slot *set = slots_[r & 1u];
        set[lane].lo.store(tag | (uint32_t)v, put);
        set[lane].hi.store(tag | (uint32_t)(v >> 32), put);
        const auto t0 = std::chrono::steady_clock::now();
        for (uint32_t l = 0; l < LANES; ++l) {
            uint64_t lo, hi;
            for (uint32_t spins = 0;; ++spins) {
                lo = set[l].lo.load(get); hi = set[l].hi.load(get);
                if ((lo >> 40) == (tag >> 40) && (hi >> 40) == (tag >> 40)) break;
                if (failed_.load()) throw Stop();
                if (left_[l].load()) {                               // (a lane deposits before it leaves: look once more)
                    lo = set[l].lo.load(get); hi = set[l].hi.load(get);
                    if ((lo >> 40) == (tag >> 40) && (hi >> 40) == (tag >> 40)) break;
                    fail("lane " + std::to_string(lane) + " waits at " + name(kind) + " for lane " + std::to_string(l) + ", which has left the walk");
                }
                if ((spins & 63u) == 63u && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(WAVE64_TIMEOUT_MS))
                    fail("lane " + std::to_string(lane) + " waited " + std::to_string(WAVE64_TIMEOUT_MS) + " ms at " + name(kind) + " for lane " + std::to_string(l));
                sched_yield();
            }
            const Kind theirs = (Kind)((lo >> 32) & 0xffu);
            if (theirs != kind)
                fail("the lanes diverged: lane " + std::to_string(lane) + " stands at " + name(kind) + ", lane " + std::to_string(l) + " at " + name(theirs));
            got[l] = (hi << 32) | (uint32_t)lo;
        }
    }

    // a lane that found the wave's lanes in disagreement at a collective of one kind
    [[noreturn]] void diverged(uint32_t lane, const std::string &what) { fail("the lanes diverged: lane " + std::to_string(lane) + " at " + what); }

private:
    struct Slot { std::atomic<uint64_t> lo{0}, hi{0}; };
    static const char *name(Kind k) {
        static const char *const n[N_KINDS] = {"ballot", "scan (32 bits)", "scan (64 bits)", "first", "bcast", "fence", "float_reserve", "float_reserve (the result)", "shfl", "readlane"};
        return k < N_KINDS ? n[k] : "?";
    }
    void stop(const std::string &why) {
        std::lock_guard<std::mutex> lk(mu_);
        if (!failed_.load()) { error_ = why; failed_.store(true); }
        main_cv_.notify_all();
    }
    [[noreturn]] void fail(const std::string &why) { stop(why); throw Stop(); }
    void lane_main(uint32_t lane) {
        uint64_t seen = 0;
        for (;;) {
            const std::function<void(uint32_t)> *body;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return quit_ || job_ != seen; });
                if (quit_) return;
                seen = job_;
                body = body_;
            }
            try { (*body)(lane); } catch (const Stop &) {}
            left_[lane].store(true);
            std::lock_guard<std::mutex> lk(mu_);
            done_.fetch_add(1u);
            main_cv_.notify_all();
        }
    }

    std::mutex mu_;                                                  // the hand-over of a body and of the message; the collectives do not take it
    std::condition_variable cv_, main_cv_;
    std::vector<std::thread> threads_;
    const std::function<void(uint32_t)> *body_ = nullptr;
    uint64_t job_ = 0;
    bool quit_ = false;
    std::string error_;
    std::atomic<uint32_t> done_{0};
    std::atomic<bool> failed_{false}, left_[LANES] = {};
    uint32_t round_[LANES] = {};                                     // per lane, touched by that lane alone
    Slot slots_[2][LANES];
};

// one lane of the wave: the W of the walks
struct Wave64Lane {
    static constexpr uint32_t LANES = Wave64::LANES;
    Wave64 *wave;
    uint32_t lane;
    uint64_t ballot(bool pred) const {
        uint64_t s[LANES], m = 0;
        wave->meet(lane, Wave64::BALLOT, pred ? 1u : 0u, s);
        for (uint32_t l = 0; l < LANES; ++l) m |= (s[l] & 1ull) << l;
        return m;
    }
    uint64_t scan(uint64_t v, uint64_t &total) const {              // exclusive prefix sum + total
        uint64_t s[LANES], below = 0, all = 0;
        wave->meet(lane, Wave64::SCAN64, v, s);
        for (uint32_t l = 0; l < LANES; ++l) { if (l < lane) below += s[l]; all += s[l]; }
        total = all;
        return below;
    }
    uint32_t scan(uint32_t v, uint32_t &total) const {
        uint64_t s[LANES];
        uint32_t below = 0, all = 0;
        wave->meet(lane, Wave64::SCAN32, v, s);
        for (uint32_t l = 0; l < LANES; ++l) { if (l < lane) below += (uint32_t)s[l]; all += (uint32_t)s[l]; }
        total = all;
        return below;
    }
    uint32_t first(bool pred) const {                                // the lowest lane with the predicate; LANES: none
        uint64_t s[LANES];
        wave->meet(lane, Wave64::FIRST, pred ? 1u : 0u, s);
        for (uint32_t l = 0; l < LANES; ++l) if (s[l]) return l;
        return LANES;
    }
    uint32_t bcast(uint32_t v, uint32_t src) const {
        uint64_t s[LANES];
        wave->meet(lane, Wave64::BCAST, v, s);
        return (uint32_t)s[src & (LANES - 1u)];
    }
    uint32_t incl_scan(uint32_t v) const { uint32_t total; return scan(v, total) + v; }     // inclusive prefix sum (32 bits, wraps like the GPU's)
    uint32_t shfl(uint32_t v, uint32_t src) const {                 // v of lane src, a source PER LANE (bcast: one source for all)
        uint64_t s[LANES];
        wave->meet(lane, Wave64::SHFL, v, s);
        return (uint32_t)s[src & (LANES - 1u)];
    }
    // v of lane n, n the same on every lane (an SGPR on the GPU): lanes that name different n have diverged, and the wave stops
    uint32_t readlane(uint32_t v, uint32_t n) const {
        uint64_t s[LANES];
        wave->meet(lane, Wave64::READLANE, (uint64_t)(n & (LANES - 1u)) << 32 | v, s);
        for (uint32_t l = 0; l < LANES; ++l)
            if ((s[l] >> 32) != (n & (LANES - 1u))) wave->diverged(lane, "readlane of lane " + std::to_string(n & (LANES - 1u)) + ", lane " + std::to_string(l) + " reads lane " + std::to_string(s[l] >> 32));
        return (uint32_t)s[n & (LANES - 1u)];
    }
    void fence() const { uint64_t s[LANES]; wave->meet(lane, Wave64::FENCE, 0u, s); }
};
