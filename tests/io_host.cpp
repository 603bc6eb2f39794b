// io_host — the host threads of the output pipeline (nanosim_amd/csrc/ns_io.h: one copier, up to 16 writers, the caller) run WITHOUT a
// GPU: ns_io.h is compiled unchanged against the runtime stub of tests/hip_host_stub, whose streams are threads, and driven through the
// same members the ns_sink_* entry points and ns_generate call (IoEngine::pick_slot / put / enqueue / drain / close / counters).
// Built plain, with -fsanitize=thread and with -fsanitize=address,undefined by tests/test_io_host.py.
//
//     io_host <scenario> [directory for the files (.)] [watchdog seconds (0 = none)]
//
// exits 0, or prints ONE line "FAIL <scenario>: ..." on the first violated expectation and exits 1 (3: the watchdog — something
// blocked).  What a file must hold comes from a sequential reference in here (a byte vector per file, filled by memcpy at the offsets
// the calls imply), never from the engine.
//
// Three witnesses of the harness sit around the engine:
//   the stub       counts a staging slice whose event is recorded again while pending, an elapsed time of an unfinished event, a
//                  stream destroyed with work, and what was never freed (hipstub::violations(), live_*())
//   pwrite         ns_io.h's pwrite is io_host_pwrite below: it counts the WRITER threads inside one descriptor at a time (the engine's
//                  "one writer per file" — overlapping pwrites at disjoint offsets leave no trace in the file), and it makes short
//                  writes, EINTR and pauses (seeded), which the loops around pwrite must absorb
//   the sanitizers on the builds that have them
#include <errno.h>
#include <fcntl.h>
#include <stdarg.h>
#include <stdio.h>
#include <sys/stat.h>
#include <unistd.h>
#include <atomic>

static ssize_t io_host_pwrite(int fd, const void *buf, size_t n, off_t off);
#define pwrite io_host_pwrite
#include "ns_io.h"
#undef pwrite

static const char *g_scn = "?";
static void failf(int line, const char *fmt, ...) __attribute__((format(printf, 2, 3), noreturn));
static void failf(int line, const char *fmt, ...) {
    char text[1024];
    va_list ap; va_start(ap, fmt); vsnprintf(text, sizeof text, fmt, ap); va_end(ap);
    printf("FAIL %s: %s (io_host.cpp:%d)\n", g_scn, text, line);
    fflush(stdout);
    _exit(1);
}
#define CHECK(cond, ...) do { if (!(cond)) failf(__LINE__, __VA_ARGS__); } while (0)

static uint64_t mix(uint64_t x) { x += 0x9E3779B97F4A7C15ull; x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull; x = (x ^ (x >> 27)) * 0x94D049BB133111EBull; return x ^ (x >> 31); }
// byte i of the pattern `key`: no period that a slice, a shifted range or another batch could share
static void fill(uint8_t *p, size_t n, uint64_t key) {
    for (size_t i = 0; i < n; i += 8) {
        const uint64_t v = mix(key * 0x100000001B3ull + i);
        memcpy(p + i, &v, std::min<size_t>(8, n - i));
    }
}

// ---- the pwrite witness ----
static thread_local bool t_caller = false;          // the thread that stands for the library's caller (ns_sink_put writes on it)
static std::atomic<int> g_inside[4096];             // writer threads inside pwrite, per descriptor
static std::atomic<uint64_t> g_two_writers{0}, g_pwrites{0};
static std::atomic<uint64_t> g_chaos{0};            // 0: plain pwrite; otherwise the seed of short writes, EINTR and pauses
static ssize_t io_host_pwrite(int fd, const void *buf, size_t n, off_t off) {
    const bool count = !t_caller && fd >= 0 && fd < 4096;
    if (count && g_inside[fd].fetch_add(1) != 0) g_two_writers++;
    const uint64_t seed = g_chaos.load(), h = seed ? mix(seed + g_pwrites++) : 0;
    ssize_t w;
    if (seed && h % 16 == 1) { errno = EINTR; w = -1; }
    else {
        if (seed && h % 4 == 2) usleep(20 + (unsigned)(h >> 8) % 80);
        w = ::pwrite(fd, buf, seed && h % 8 == 0 && n > 1 ? n / 2 : n, off);
    }
    if (count) g_inside[fd].fetch_sub(1);
    return w;
}

// ---- the reference: what each file must hold ----
struct File {
    std::string path;
    int fd = -1;
    ns_sink *s = nullptr;
    uint64_t off = 0, total = 0;          // the harness's own account: offset of the next byte, bytes given to the sink
    std::vector<uint8_t> ref;
    void expect(const void *src, uint64_t n) {
        if (n) { if (ref.size() < off + n) ref.resize(off + n); memcpy(&ref[off], src, n); }
        off += n; total += n;
    }
    void create(const std::string &p, uint64_t off0) {
        path = p; off = off0;
        fd = open(p.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
        CHECK(fd >= 0, "open %s: %s", p.c_str(), strerror(errno));
    }
    // the file against the reference, byte for byte; then gone
    void verify_and_remove() {
        if (fd >= 0) { ::close(fd); fd = -1; }
        FILE *f = fopen(path.c_str(), "rb");
        CHECK(f, "reopen %s: %s", path.c_str(), strerror(errno));
        std::vector<uint8_t> got(ref.size() + 1);
        const size_t n = fread(got.data(), 1, got.size(), f);
        fclose(f);
        CHECK(n == ref.size(), "%s holds %zu bytes, the reference %zu", path.c_str(), n, ref.size());
        for (size_t i = 0; i < n; ++i)
            CHECK(got[i] == ref[i], "%s differs from the reference at byte %zu of %zu: 0x%02x, expected 0x%02x", path.c_str(), i, n, got[i], ref[i]);
        unlink(path.c_str());
    }
};

// ---- the engine as a context holds it ----
static const size_t SLICE = 4096;
struct Rig {
    IoEngine *io = nullptr;
    std::vector<ns_sink *> sinks;         // (ns_ctx::sinks)
    int slot = 0;                         // (ns_ctx::slot)
    std::string msg;
    static void knobs(size_t slices, size_t threads) {
        setenv("NS_IO_SLICE_BYTES", std::to_string(SLICE).c_str(), 1);
        setenv("NS_IO_SLICES", std::to_string(slices).c_str(), 1);
        setenv("NS_IO_THREADS", std::to_string(threads).c_str(), 1);
    }
    void start(size_t slices, size_t threads) {
        knobs(slices, threads);
        io = new IoEngine();
        const int rc = io->start(0, msg);
        CHECK(rc == 0, "start(%zu slices, %zu threads) returned %d: %s", slices, threads, rc, msg.c_str());
        ns_io_stats c; io->counters(&c, 0);
        CHECK(c.n_slices == slices && c.n_threads == threads && c.slice_bytes == SLICE, "counters: %u slices, %u threads, slices of %llu bytes",
              c.n_slices, c.n_threads, (unsigned long long)c.slice_bytes);
    }
    ns_sink *open(int fd, uint64_t off) {          // (the three lines of ns_sink_open behind its argument checks)
        ns_sink *s = new ns_sink();
        s->fd = fd; s->off = off;
        sinks.push_back(s);
        return s;
    }
    void attach(File &f) { f.s = open(f.fd, f.off); }
    // result slot of the next batch, as ns_generate chooses it
    int next_slot() { return slot = io->pick_slot(slot); }
    void put(File &f, const void *p, uint64_t n) {
        const int rc = IoEngine::put(f.s, p, n, msg);
        CHECK(rc == NS_OK, "put of %llu bytes into %s returned %d: %s", (unsigned long long)n, f.path.c_str(), rc, msg.c_str());
        f.expect(p, n);
    }
    void queue(File &f, const uint8_t *p, uint64_t n) { io->enqueue(f.s, p, n, slot); f.expect(p, n); }
    void drain_ok(File &f) {
        uint64_t off = ~0ull;
        const int rc = io->drain(f.s, &off, msg);
        CHECK(rc == NS_OK, "drain of %s returned %d: %s", f.path.c_str(), rc, msg.c_str());
        CHECK(off == f.off, "drain of %s: file offset %llu, expected %llu", f.path.c_str(), (unsigned long long)off, (unsigned long long)f.off);
        CHECK(f.s->queued.load() == f.total && f.s->written.load() == f.total, "%s: queued %llu, written %llu, given %llu", f.path.c_str(),
              (unsigned long long)f.s->queued.load(), (unsigned long long)f.s->written.load(), (unsigned long long)f.total);
    }
    void close_ok(File &f) {
        const size_t before = sinks.size();
        const int rc = io->close(sinks, f.s, msg);
        f.s = nullptr;
        CHECK(rc == NS_OK, "close of %s returned %d: %s", f.path.c_str(), rc, msg.c_str());
        CHECK(sinks.size() + 1 == before, "close of %s left %zu of %zu sinks", f.path.c_str(), sinks.size(), before);
    }
    void stop() {                                  // (ns_destroy)
        io->wait_all(); io->shutdown(); delete io; io = nullptr;
        for (ns_sink *s : sinks) delete s;
        sinks.clear();
    }
};

static void check_clean(const char *where) {
    CHECK(hipstub::violations() == 0, "%s: the runtime stub counted %llu violations, the first: %s", where, (unsigned long long)hipstub::violations(),
          hipstub::first_violation());
    CHECK(g_two_writers.load() == 0, "%s: %llu times a second writer thread was inside pwrite for the same file", where, (unsigned long long)g_two_writers.load());
    CHECK(hipstub::live_host_allocs() == 0 && hipstub::live_streams() == 0 && hipstub::live_events() == 0,
          "%s: left behind: %ld staging allocations, %ld streams, %ld events", where, hipstub::live_host_allocs(), hipstub::live_streams(), hipstub::live_events());
}
static void fresh(uint64_t seed, unsigned max_delay_us) {
    hipstub::reset();
    hipstub::set_delay(seed, max_delay_us);
    g_chaos = seed; g_pwrites = 0;
}

// ---- a. round trip ----
static void scn_roundtrip(const std::string &dir) {
    const size_t sizes[] = {0, 1, SLICE - 1, SLICE, SLICE + 1, 3 * SLICE + 5};
    const size_t n_sizes = sizeof sizes / sizeof *sizes;
    uint64_t combo = 0;
    for (size_t n_slices : {1, 3, 24}) for (size_t n_threads : {1, 4, 16}) for (size_t n_sinks : {1, 2, 7, 33}) {        // 33: NS_IO_FANOUT + 1
        ++combo;
        char where[96]; snprintf(where, sizeof where, "%zu slices, %zu threads, %zu sinks", n_slices, n_threads, n_sinks);
        fresh(combo, combo % 3 == 0 ? 0 : 40);
        Rig r; r.start(n_slices, n_threads);
        std::vector<File> files(n_sinks);
        for (size_t k = 0; k < n_sinks; ++k) { files[k].create(dir + "/rt" + std::to_string(k), 1000 + 37 * k); r.attach(files[k]); }      // initial offset non-zero
        std::vector<std::vector<uint8_t>> bufs(n_sizes);              // (they stand for device memory: alive until their copies have run)
        uint64_t queued = 0, want_slices = 0, counted = 0;
        ns_io_stats c;
        for (size_t round = 0; round < n_sizes; ++round) {
            const size_t n = sizes[round];
            bufs[round].resize(n + n_sinks);
            fill(bufs[round].data(), bufs[round].size(), combo * 100 + round);
            r.next_slot();
            for (size_t k = 0; k < n_sinks; ++k) {
                char hdr[48]; const int h = snprintf(hdr, sizeof hdr, "#sink %zu round %zu\n", k, round);
                r.put(files[k], hdr, (uint64_t)h);                    // a header between queued buffers of the same sink
                r.queue(files[k], bufs[round].data() + k, n);         // (shifted by k: every sink its own bytes)
                queued += n; want_slices += (n + SLICE - 1) / SLICE;
            }
            r.io->counters(&c, 1); counted += c.bytes;                // read and reset on the calling thread, slices in flight
            CHECK(c.n_slices == n_slices, "%s: counters report %u slices", where, c.n_slices);
        }
        for (File &f : files) r.drain_ok(f);
        r.io->counters(&c, 1); counted += c.bytes;
        CHECK(counted == queued, "%s: the counters saw %llu bytes, %llu were queued", where, (unsigned long long)counted, (unsigned long long)queued);
        CHECK(c.dma_ms >= 0 && c.write_s >= 0 && c.wait_staging_s >= 0, "%s: a negative time in the counters", where);
        r.io->counters(&c, 0);
        CHECK(c.bytes == 0 && c.dma_ms == 0, "%s: counters not zero after a reset: %llu bytes", where, (unsigned long long)c.bytes);
        CHECK(hipstub::memcpy_calls() == want_slices && hipstub::memcpy_bytes() == queued, "%s: %llu copies of %llu bytes, expected %llu of %llu", where,
              (unsigned long long)hipstub::memcpy_calls(), (unsigned long long)hipstub::memcpy_bytes(), (unsigned long long)want_slices, (unsigned long long)queued);
        for (File &f : files) r.close_ok(f);
        r.stop();
        check_clean(where);
        for (File &f : files) f.verify_and_remove();
    }
}

// ---- b. slot reuse: a result slot is overwritten only when its copies have left it ----
static void slot_reuse_run(const std::string &dir, size_t n_slices, size_t n_threads, unsigned batches, uint64_t seed) {
    const size_t cap = 2 * SLICE + 77;
    fresh(seed, 200);
    Rig r; r.start(n_slices, n_threads);
    std::vector<uint8_t> slot_buf[2] = {std::vector<uint8_t>(cap), std::vector<uint8_t>(cap)};
    File f[3];
    for (int k = 0; k < 3; ++k) { f[k].create(dir + "/slot" + std::to_string(k), k ? 0 : 11); r.attach(f[k]); }
    for (unsigned b = 0; b < batches; ++b) {
        const int slot = r.next_slot();                                // slot_busy -> flip, then wait_slot
        uint8_t *p = slot_buf[slot].data();
        fill(p, cap, seed * 100000 + b);                               // "ns_generate": the whole buffer, this batch's pattern
        const size_t n = b % 17 == 16 ? 0 : cap - (b * 37) % 700, cut = (b * 131) % (n + 1);
        r.queue(f[0], p, n);                                           // the image
        r.queue(f[1], p + n / 3, n / 2);                               // a sub-range
        r.queue(f[2], p, cut); r.queue(f[2], p + cut, n - cut);       // cut in two at a "read boundary", as the sub-files of -t K
    }
    for (File &x : f) r.drain_ok(x);
    for (File &x : f) r.close_ok(x);
    r.stop();
    check_clean("slot reuse");
    for (File &x : f) x.verify_and_remove();
}
static void scn_slot_reuse(const std::string &dir) {
    slot_reuse_run(dir, 3, 4, 200, 1);
    slot_reuse_run(dir, 24, 16, 100, 2);      // every slice of a batch in flight at once
    slot_reuse_run(dir, 1, 1, 40, 3);
}

// ---- c. sinks without a file ----
static void scn_no_file(const std::string &dir) {
    fresh(7, 40);
    Rig r; r.start(3, 4);
    const size_t n = 3 * SLICE + 5;
    std::vector<uint8_t> buf(n);
    fill(buf.data(), n, 7);
    File drop, null, real;
    drop.path = "(no descriptor)"; drop.off = 5;
    null.path = "/dev/null"; null.fd = open("/dev/null", O_WRONLY);
    CHECK(null.fd >= 0, "open /dev/null: %s", strerror(errno));
    real.create(dir + "/nofile_real", 0);
    r.attach(drop); r.attach(null); r.attach(real);
    for (int round = 0; round < 3; ++round) {
        r.next_slot();
        for (File *f : {&drop, &null, &real}) { r.put(*f, "header\n", 7); r.queue(*f, buf.data(), n); }
    }
    for (File *f : {&drop, &null, &real}) r.drain_ok(*f);
    ns_io_stats c; r.io->counters(&c, 0);
    CHECK(c.bytes == 9 * n, "counters: %llu bytes, expected %llu", (unsigned long long)c.bytes, (unsigned long long)(9 * n));
    for (File *f : {&drop, &null, &real}) r.close_ok(*f);
    r.stop();
    ::close(null.fd);
    check_clean("no file");
    real.verify_and_remove();
}

// ---- d. failed writes ----
static void failed_writes_run(const std::string &dir, size_t n_slices, size_t n_threads, uint64_t seed) {
    fresh(seed, 40);
    Rig r; r.start(n_slices, n_threads);
    const size_t n = 3 * SLICE + 5, rounds = 6;
    File good[3], full, closed;
    for (int k = 0; k < 3; ++k) good[k].create(dir + "/fw_good" + std::to_string(k), 3 * k);
    full.path = "/dev/full"; full.fd = open("/dev/full", O_WRONLY);
    CHECK(full.fd >= 0, "open /dev/full: %s", strerror(errno));
    closed.create(dir + "/fw_closed", 0);
    File *order[] = {&good[0], &full, &good[1], &closed, &good[2]};
    for (File *f : order) r.attach(*f);
    ::close(closed.fd);                   // closed under its sink; no descriptor is opened from here to the end of the engine (the number stays free)
    std::vector<std::vector<uint8_t>> bufs(rounds, std::vector<uint8_t>(n + 5));
    for (size_t round = 0; round < rounds; ++round) {
        fill(bufs[round].data(), n + 5, seed * 1000 + round);
        r.next_slot();
        for (int k = 0; k < 5; ++k) {
            if (order[k] != &full && order[k] != &closed) r.put(*order[k], "ok\n", 3);
            r.queue(*order[k], bufs[round].data() + k, n);
        }
    }
    struct { File *f; int err; } bad[] = {{&full, ENOSPC}, {&closed, EBADF}};
    for (auto &b : bad) {
        uint64_t off = 0;
        const int rc = r.io->drain(b.f->s, &off, r.msg);              // returns: the later slices are skipped, and still accounted
        CHECK(rc == NS_EIO && r.msg == std::string("write: ") + strerror(b.err), "drain of %s returned %d \"%s\", expected NS_EIO \"write: %s\"",
              b.f->path.c_str(), rc, r.msg.c_str(), strerror(b.err));
        CHECK(b.f->s->err.load() == b.err, "%s: errno %d, expected %d", b.f->path.c_str(), b.f->s->err.load(), b.err);
        CHECK(off == b.f->off && b.f->s->written.load() == b.f->total && b.f->s->queued.load() == b.f->total, "%s: offset %llu, written %llu of %llu",
              b.f->path.c_str(), (unsigned long long)off, (unsigned long long)b.f->s->written.load(), (unsigned long long)b.f->total);
    }
    {   // a put into the full file fails on the caller's thread and moves nothing
        const uint64_t q = full.s->queued.load(), o = full.s->off;
        const int rc = IoEngine::put(full.s, "x", 1, r.msg);
        CHECK(rc == NS_EIO && r.msg == std::string("write: ") + strerror(ENOSPC), "put into /dev/full returned %d \"%s\"", rc, r.msg.c_str());
        CHECK(full.s->queued.load() == q && full.s->off == o, "a failed put moved the sink's offset");
    }
    for (File &f : good) r.drain_ok(f);
    ns_io_stats c; r.io->counters(&c, 0);
    CHECK(c.bytes == 5 * rounds * n, "counters: %llu bytes, expected %llu", (unsigned long long)c.bytes, (unsigned long long)(5 * rounds * n));
    for (auto &b : bad) {                 // close reports the same error and still forgets the sink
        const size_t before = r.sinks.size();
        const int rc = r.io->close(r.sinks, b.f->s, r.msg);
        CHECK(rc == NS_EIO && r.sinks.size() + 1 == before, "close of %s returned %d, %zu of %zu sinks left", b.f->path.c_str(), rc, r.sinks.size(), before);
    }
    for (File &f : good) r.close_ok(f);
    r.stop();
    ::close(full.fd);
    check_clean("failed writes");
    for (File &f : good) f.verify_and_remove();
    unlink(closed.path.c_str());
}
static void scn_failed_writes(const std::string &dir) {
    failed_writes_run(dir, 3, 4, 11);
    failed_writes_run(dir, 24, 16, 12);
    failed_writes_run(dir, 1, 1, 13);
}

// ---- e. copy-side failures ----
static void copy_failures_run(const std::string &dir, int mode) {
    fresh(20 + (uint64_t)mode, 40);
    Rig r; r.start(3, 4);
    const size_t n = 3 * SLICE + 5, rounds = 4;
    File f[3];
    for (int k = 0; k < 3; ++k) { f[k].create(dir + "/cf" + std::to_string(k), 0); r.attach(f[k]); }
    std::vector<std::vector<uint8_t>> bufs(rounds + 1, std::vector<uint8_t>(n + 3));
    fill(bufs[rounds].data(), n + 3, 99);
    r.next_slot();
    for (int k = 0; k < 3; ++k) r.queue(f[k], bufs[rounds].data() + k, n);
    for (File &x : f) r.drain_ok(x);      // a healthy round first
    std::string want;
    if (mode == 0) { hipstub::fail_memcpy_at(5, hipErrorStubInjectedA); want = std::string("ns_io: device-to-host copy: ") + hipstub::INJECTED_A; }
    if (mode == 1) { hipstub::fail_event_sync_at(5, hipErrorStubInjectedB); want = std::string("ns_io: copy event: ") + hipstub::INJECTED_B; }
    if (mode == 2) {                      // two failures: the message of the first one stays (copy 3 is issued before a ninth event can be waited for)
        hipstub::fail_memcpy_at(3, hipErrorStubInjectedA); hipstub::fail_event_sync_at(9, hipErrorStubInjectedB);
        want = std::string("ns_io: device-to-host copy: ") + hipstub::INJECTED_A;
    }
    for (size_t round = 0; round < rounds; ++round) {
        fill(bufs[round].data(), n + 3, (uint64_t)mode * 10 + round);
        r.next_slot();
        for (int k = 0; k < 3; ++k) r.io->enqueue(f[k].s, bufs[round].data() + k, n, r.slot);
    }
    r.io->wait_slot(0); r.io->wait_slot(1);
    for (File &x : f) r.io->wait_sink(x.s);
    r.io->wait_all();
    for (File &x : f) {
        const int rc = r.io->drain(x.s, nullptr, r.msg);
        CHECK(rc == NS_EHIP && r.msg == want, "mode %d: drain returned %d \"%s\", expected NS_EHIP \"%s\"", mode, rc, r.msg.c_str(), want.c_str());
        CHECK(x.s->written.load() == x.s->queued.load() && x.s->queued.load() == (rounds + 1) * n, "mode %d: written %llu of %llu", mode,
              (unsigned long long)x.s->written.load(), (unsigned long long)x.s->queued.load());
    }
    { std::lock_guard<std::mutex> g(r.io->mu); CHECK(r.io->err == want, "mode %d: the engine's error is \"%s\"", mode, r.io->err.c_str()); }
    for (File &x : f) {
        const int rc = r.io->close(r.sinks, x.s, r.msg);
        CHECK(rc == NS_EHIP, "mode %d: close returned %d", mode, rc);
    }
    r.stop();
    check_clean("copy failures");
    for (File &x : f) { ::close(x.fd); unlink(x.path.c_str()); }
}
static void scn_copy_failures(const std::string &dir) { for (int mode = 0; mode < 3; ++mode) copy_failures_run(dir, mode); }

// ---- f. start-up failures ----
static void scn_startup_failures(const std::string &) {
    for (int which = 0; which < 4; ++which) {
        fresh(0, 0);
        Rig::knobs(24, 16);
        const char *want = which == 0 ? "ns_io: no copy stream" : "ns_io: staging allocation failed";
        if (which == 0) hipstub::fail_stream_create(true);
        else hipstub::fail_host_malloc_at(which == 1 ? 1 : which == 2 ? 12 : 24);      // slice 0, in the middle, the last one
        IoEngine *io = new IoEngine();
        std::string msg;
        const int rc = io->start(0, msg);                             // (ns_sink_open: start fails -> shutdown, delete)
        CHECK(rc == -1 && msg == want, "case %d: start returned %d \"%s\", expected -1 \"%s\"", which, rc, msg.c_str(), want);
        CHECK(!io->copier.joinable() && io->writers.empty(), "case %d: threads were started", which);
        io->shutdown();
        delete io;
        hipstub::fail_stream_create(false);
        check_clean(want);
    }
}

// ---- g. lifetime churn: close deletes a sink right after the wait ----
static void scn_churn(const std::string &dir) {
    for (int i = 0; i < 20; ++i) {        // shutdown straight after start
        fresh(0, 0);
        Rig r; r.start(i % 2 ? 24 : 2, i % 3 ? 16 : 1);
        r.io->shutdown(); delete r.io;
    }
    {                                     // sinks, and nothing ever queued
        fresh(0, 0);
        Rig r; r.start(3, 4);
        File a, b; a.create(dir + "/churn_idle", 0); b.path = "(no descriptor)";
        r.attach(a); r.attach(b);
        r.drain_ok(a); r.close_ok(a);
        r.stop();                         // (b is still open: ns_destroy deletes it)
        a.verify_and_remove();
    }
    check_clean("idle engines");
    fresh(31, 30);
    Rig r; r.start(6, 8);
    const size_t cap = 4 * SLICE;
    std::vector<uint8_t> slot_buf[2] = {std::vector<uint8_t>(cap), std::vector<uint8_t>(cap)};
    File longlived[3];
    for (int k = 0; k < 3; ++k) { longlived[k].create(dir + "/churn_long" + std::to_string(k), 0); r.attach(longlived[k]); }
    for (unsigned i = 0; i < 1000; ++i) {
        const int slot = r.next_slot();
        uint8_t *p = slot_buf[slot].data();
        fill(p, cap, 5000000 + i);
        File s;
        s.create(dir + "/churn_short", i % 3 ? 0 : 17);
        r.attach(s);
        r.queue(s, p + i % 7, (1 + i % 3) * SLICE - i % 5);            // one to three slices
        r.queue(longlived[i % 3], p + SLICE / 2, SLICE + i % 9);       // other files' slices complete (and wake the waiter) meanwhile
        r.queue(longlived[(i + 1) % 3], p, 3 * SLICE - i % 11);
        r.close_ok(s);                                                 // wait_sink, then delete
        s.verify_and_remove();
    }
    r.io->wait_all();
    for (File &f : longlived) { r.drain_ok(f); r.close_ok(f); }
    r.stop();
    check_clean("churn");
    for (File &f : longlived) f.verify_and_remove();
}

// ---- the stub itself: what it calls a violation, it does count ----
static void scn_stub_strict(const std::string &) {
    fresh(0, 0);
    hipstub::quiet(true);
    hipStream_t q; hipEvent_t ev, never;
    CHECK(hipStreamCreateWithFlags(&q, hipStreamNonBlocking) == hipSuccess && hipEventCreate(&ev) == hipSuccess && hipEventCreate(&never) == hipSuccess, "stub objects");
    float ms = -1;
    uint8_t src[64], dst[64] = {0};
    fill(src, sizeof src, 1);
    hipstub::hold_streams(true);
    CHECK(hipEventRecord(ev, q) == hipSuccess && hipMemcpyAsync(dst, src, sizeof src, hipMemcpyDeviceToHost, q) == hipSuccess, "enqueue");
    CHECK(hipstub::violations() == 0 && dst[0] == 0 && dst[63] == 0, "a copy ran at the call, not on the stream");
    hipEventRecord(ev, q);
    CHECK(hipstub::violations() == 1, "an event recorded again while pending was not counted");
    CHECK(hipEventElapsedTime(&ms, ev, ev) == hipErrorNotReady && hipstub::violations() == 2, "the elapsed time of a pending event was not counted");
    CHECK(hipEventElapsedTime(&ms, never, ev) == hipErrorInvalidHandle && hipstub::violations() == 3, "the elapsed time of an event never recorded was not counted");
    hipstub::hold_streams(false);
    CHECK(hipEventSynchronize(ev) == hipSuccess && hipStreamSynchronize(q) == hipSuccess && !memcmp(src, dst, sizeof src), "the copy did not arrive");
    CHECK(hipEventElapsedTime(&ms, ev, ev) == hipSuccess && ms == 0 && hipstub::violations() == 3, "elapsed time of a completed event");
    hipstub::hold_streams(true);
    hipEventRecord(ev, q);
    hipStreamDestroy(q);
    CHECK(hipstub::violations() == 4, "a stream destroyed with queued work was not counted");
    hipstub::hold_streams(false);
    hipEventDestroy(ev); hipEventDestroy(never);
    CHECK(hipstub::violations() == 4 && hipstub::live_streams() == 0 && hipstub::live_events() == 0, "stub objects left");
    CHECK(!strcmp(hipGetErrorString(hipErrorStubInjectedA), hipstub::INJECTED_A) && strcmp(hipstub::INJECTED_A, hipstub::INJECTED_B), "error strings");
    hipstub::reset();
}

// ---- main: one scenario, under a watchdog ----
// (the watchdog polls: a timed wait on a condition variable goes through pthread_cond_clockwait, which older ThreadSanitizer
// runtimes do not know — they report the mutex as locked twice)
static std::atomic<bool> g_wd_done{false};

int main(int argc, char **argv) {
    static const struct { const char *name; void (*run)(const std::string &); } scenarios[] = {
        {"roundtrip", scn_roundtrip}, {"slot_reuse", scn_slot_reuse}, {"no_file", scn_no_file}, {"failed_writes", scn_failed_writes},
        {"copy_failures", scn_copy_failures}, {"startup_failures", scn_startup_failures}, {"churn", scn_churn}, {"stub_strict", scn_stub_strict}};
    if (argc < 2) {
        for (auto &s : scenarios) puts(s.name);
        return 2;
    }
    const std::string dir = argc > 2 ? argv[2] : ".";
    const int limit = argc > 3 ? atoi(argv[3]) : 0;
    t_caller = true;
    for (auto &s : scenarios) {
        if (strcmp(s.name, argv[1])) continue;
        g_scn = s.name;
        std::thread watchdog;
        if (limit > 0) watchdog = std::thread([limit] {
            const auto end = std::chrono::steady_clock::now() + std::chrono::seconds(limit);
            while (std::chrono::steady_clock::now() < end) {
                if (g_wd_done.load()) return;
                usleep(20000);
            }
            printf("FAIL %s: still running after %d s: a thread waits for something that does not come\n", g_scn, limit);
            fflush(stdout);
            _exit(3);
        });
        s.run(dir);
        if (watchdog.joinable()) {
            g_wd_done = true;
            watchdog.join();
        }
        printf("ok %s\n", s.name);
        return 0;
    }
    printf("FAIL %s: no such scenario\n", argv[1]);
    return 2;
}
