// The runtime calls of hip/hip_runtime.h (this directory) on host threads: see the header for what the stub is for.
//
// One mutex guards all of the stub's state, and one condition variable wakes whoever waits for it to change: the stub is about
// ORDER, not speed.  The copy itself (memcpy) runs on the stream's thread with the mutex released — ThreadSanitizer then sees the
// read of the source and the write of the staging slice as plain accesses of that thread, ordered against the engine's threads
// only through what the engine itself waits for (hipEventSynchronize, hipStreamSynchronize).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <set>
#include <string>
#include <thread>

namespace {
struct Op { int kind; void *dst; const void *src; size_t n; hipstub_event *ev; };      // kind 0: copy, 1: event record
enum { OP_COPY = 0, OP_RECORD = 1 };
}

struct hipstub_event {
    unsigned pending = 0;                  // records enqueued and not yet run
    bool recorded = false;                 // has been recorded at least once
    std::chrono::steady_clock::time_point at;      // when its last record ran
};
struct hipstub_stream {
    std::deque<Op> fifo;
    bool running = false;                  // an operation has been taken off the FIFO and has not finished
    bool quit = false;
    uint64_t rng = 0;
    std::thread th;
};

namespace {
struct State {
    std::mutex mu;
    std::condition_variable cv;
    std::set<void *> host_allocs;
    long streams = 0, events = 0;
    uint64_t seed = 0; unsigned max_us = 0;
    uint64_t n_memcpy = 0, n_memcpy_bytes = 0, n_sync = 0, n_malloc = 0;
    uint64_t fail_memcpy = 0, fail_sync = 0, fail_malloc = 0;
    hipError_t fail_memcpy_code = hipSuccess, fail_sync_code = hipSuccess;
    bool fail_stream = false;
    bool hold = false, quiet = false;
    uint64_t n_violations = 0;
    std::string first;
};
State &st() { static State *s = new State(); return *s; }       // never destroyed: stream threads may outlive main's statics

// (with the mutex held)
void violation(State &s, const char *what) {
    if (!s.n_violations++) s.first = what;
    if (!s.quiet) fprintf(stderr, "hip_stub: VIOLATION: %s\n", what);
}
uint64_t next_rand(uint64_t &x) { x += 0x9E3779B97F4A7C15ull; uint64_t z = x; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }

void stream_loop(hipstub_stream *q) {
    State &s = st();
    std::unique_lock<std::mutex> g(s.mu);
    for (;;) {
        s.cv.wait(g, [&] { return q->quit || (!s.hold && !q->fifo.empty()); });
        if (q->fifo.empty()) return;
        const Op op = q->fifo.front(); q->fifo.pop_front();
        q->running = true;
        const unsigned us = s.max_us ? (unsigned)(next_rand(q->rng) % (s.max_us + 1)) : 0;
        g.unlock();
        if (us) std::this_thread::sleep_for(std::chrono::microseconds(us));
        if (op.kind == OP_COPY) memcpy(op.dst, op.src, op.n);
        g.lock();
        if (op.kind == OP_RECORD) { op.ev->at = std::chrono::steady_clock::now(); --op.ev->pending; }
        q->running = false;
        s.cv.notify_all();
    }
}
}  // namespace

hipError_t hipSetDevice(int) { return hipSuccess; }

hipError_t hipStreamCreateWithFlags(hipStream_t *stream, unsigned) {
    State &s = st();
    std::lock_guard<std::mutex> g(s.mu);
    if (s.fail_stream) return hipErrorOutOfMemory;
    hipstub_stream *q = new hipstub_stream();
    q->rng = s.seed ^ (0x51ED270B1ull * (uint64_t)(++s.streams));
    q->th = std::thread(stream_loop, q);
    *stream = q;
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t q) {
    State &s = st();
    std::unique_lock<std::mutex> g(s.mu);
    s.cv.wait(g, [&] { return q->fifo.empty() && !q->running; });
    return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t q) {
    State &s = st();
    {
        std::lock_guard<std::mutex> g(s.mu);
        if (!q->fifo.empty() || q->running) violation(s, "hipStreamDestroy: the stream still has queued work");
        q->quit = true;
    }
    s.cv.notify_all();
    q->th.join();                          // (what was queued still runs: its buffers may be freed right after this call)
    { std::lock_guard<std::mutex> g(s.mu); --s.streams; }
    delete q;
    return hipSuccess;
}

hipError_t hipHostMalloc(void **ptr, size_t size, unsigned) {
    State &s = st();
    std::lock_guard<std::mutex> g(s.mu);
    if (++s.n_malloc == s.fail_malloc) { *ptr = nullptr; return hipErrorOutOfMemory; }
    void *p = malloc(size ? size : 1);
    if (!p) { *ptr = nullptr; return hipErrorOutOfMemory; }
    s.host_allocs.insert(p);
    *ptr = p;
    return hipSuccess;
}
hipError_t hipHostFree(void *p) {
    State &s = st();
    {
        std::lock_guard<std::mutex> g(s.mu);
        if (!s.host_allocs.erase(p)) { fprintf(stderr, "hip_stub: hipHostFree(%p): not a pointer of hipHostMalloc (or freed twice)\n", p); abort(); }
    }
    free(p);
    return hipSuccess;
}

hipError_t hipEventCreate(hipEvent_t *ev) {
    State &s = st();
    std::lock_guard<std::mutex> g(s.mu);
    *ev = new hipstub_event();
    ++s.events;
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t ev) {
    State &s = st();
    std::unique_lock<std::mutex> g(s.mu);
    if (ev->pending) {
        violation(s, "hipEventDestroy: the event is still pending");
        s.cv.wait(g, [&] { return ev->pending == 0; });      // (the stream's thread still holds the pointer)
    }
    --s.events;
    delete ev;
    return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t ev, hipStream_t q) {
    State &s = st();
    {
        std::lock_guard<std::mutex> g(s.mu);
        if (ev->pending) violation(s, "hipEventRecord: the event is still pending from an earlier record (a staging slice reused before its copy finished)");
        ++ev->pending; ev->recorded = true;
        q->fifo.push_back(Op{OP_RECORD, nullptr, nullptr, 0, ev});
    }
    s.cv.notify_all();
    return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t ev) {
    State &s = st();
    std::unique_lock<std::mutex> g(s.mu);
    const bool inject = ++s.n_sync == s.fail_sync;
    s.cv.wait(g, [&] { return ev->pending == 0; });
    return inject ? s.fail_sync_code : hipSuccess;
}
hipError_t hipEventElapsedTime(float *ms, hipEvent_t a, hipEvent_t b) {
    State &s = st();
    std::lock_guard<std::mutex> g(s.mu);
    if (!a->recorded || !b->recorded) { violation(s, "hipEventElapsedTime: an event that was never recorded"); return hipErrorInvalidHandle; }
    if (a->pending || b->pending) { violation(s, "hipEventElapsedTime: an event that has not completed"); return hipErrorNotReady; }
    *ms = std::chrono::duration<float, std::milli>(b->at - a->at).count();
    return hipSuccess;
}

hipError_t hipMemcpyAsync(void *dst, const void *src, size_t n, hipMemcpyKind, hipStream_t q) {
    State &s = st();
    {
        std::lock_guard<std::mutex> g(s.mu);
        if (++s.n_memcpy == s.fail_memcpy) return s.fail_memcpy_code;
        s.n_memcpy_bytes += n;
        q->fifo.push_back(Op{OP_COPY, dst, src, n, nullptr});
    }
    s.cv.notify_all();
    return hipSuccess;
}

const char *hipGetErrorString(hipError_t e) {
    switch (e) {
    case hipSuccess: return "no error";
    case hipErrorInvalidValue: return "invalid argument";
    case hipErrorOutOfMemory: return "out of memory";
    case hipErrorInvalidHandle: return "invalid resource handle";
    case hipErrorNotReady: return "device not ready";
    case hipErrorStubInjectedA: return hipstub::INJECTED_A;
    case hipErrorStubInjectedB: return hipstub::INJECTED_B;
    }
    return "unknown error";
}

namespace hipstub {
const char *const INJECTED_A = "hip_stub injected failure A";
const char *const INJECTED_B = "hip_stub injected failure B";
void reset() {
    State &s = st();
    std::lock_guard<std::mutex> g(s.mu);
    s.seed = 0; s.max_us = 0;
    s.n_memcpy = s.n_memcpy_bytes = s.n_sync = s.n_malloc = 0;
    s.fail_memcpy = s.fail_sync = s.fail_malloc = 0;
    s.fail_stream = false;
    s.hold = s.quiet = false;
    s.n_violations = 0; s.first.clear();
}
void set_delay(uint64_t seed, unsigned max_us) { State &s = st(); std::lock_guard<std::mutex> g(s.mu); s.seed = seed; s.max_us = max_us; }
void fail_memcpy_at(uint64_t nth, hipError_t code) { State &s = st(); std::lock_guard<std::mutex> g(s.mu); s.fail_memcpy = nth ? s.n_memcpy + nth : 0; s.fail_memcpy_code = code; }
void fail_event_sync_at(uint64_t nth, hipError_t code) { State &s = st(); std::lock_guard<std::mutex> g(s.mu); s.fail_sync = nth ? s.n_sync + nth : 0; s.fail_sync_code = code; }
void fail_host_malloc_at(uint64_t nth) { State &s = st(); std::lock_guard<std::mutex> g(s.mu); s.fail_malloc = nth ? s.n_malloc + nth : 0; }
void hold_streams(bool on) { State &s = st(); { std::lock_guard<std::mutex> g(s.mu); s.hold = on; } s.cv.notify_all(); }
void quiet(bool on) { State &s = st(); std::lock_guard<std::mutex> g(s.mu); s.quiet = on; }
void fail_stream_create(bool on) { State &s = st(); std::lock_guard<std::mutex> g(s.mu); s.fail_stream = on; }
uint64_t memcpy_calls() { State &s = st(); std::lock_guard<std::mutex> g(s.mu); return s.n_memcpy; }
uint64_t memcpy_bytes() { State &s = st(); std::lock_guard<std::mutex> g(s.mu); return s.n_memcpy_bytes; }
uint64_t event_sync_calls() { State &s = st(); std::lock_guard<std::mutex> g(s.mu); return s.n_sync; }
uint64_t violations() { State &s = st(); std::lock_guard<std::mutex> g(s.mu); return s.n_violations; }
const char *first_violation() { State &s = st(); std::lock_guard<std::mutex> g(s.mu); return s.first.c_str(); }
long live_host_allocs() { State &s = st(); std::lock_guard<std::mutex> g(s.mu); return (long)s.host_allocs.size(); }
long live_streams() { State &s = st(); std::lock_guard<std::mutex> g(s.mu); return s.streams; }
long live_events() { State &s = st(); std::lock_guard<std::mutex> g(s.mu); return s.events; }
}  // namespace hipstub
