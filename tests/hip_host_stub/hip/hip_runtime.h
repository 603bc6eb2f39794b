// A stand-in for <hip/hip_runtime.h>, for the host-only test programs of the output pipeline (tests/io_host.cpp): it declares the
// runtime entry points that nanosim_amd/csrc/ns_io.h calls and nothing else, so that ns_io.h compiles UNCHANGED with a plain g++
// and runs on a machine without a GPU — under ThreadSanitizer and AddressSanitizer, which see host threads and host memory only.
// tests/hip_host_stub/hip_stub.cpp implements them; the product's build never has this directory on its include path.
//
// The stub is ASYNCHRONOUS like the real runtime — a stream is a thread with a FIFO of operations; hipMemcpyAsync and
// hipEventRecord enqueue and return, the copy runs later — and STRICT about use: what the real runtime would answer with an error
// code or with undefined behaviour is counted as a violation that the test program reads at its end (hipstub::violations()).
#pragma once
#include <stddef.h>
#include <stdint.h>

typedef enum hipError_t {
    hipSuccess = 0,
    hipErrorInvalidValue = 1,
    hipErrorOutOfMemory = 2,
    hipErrorInvalidHandle = 400,
    hipErrorNotReady = 600,
    hipErrorStubInjectedA = 9001,          // the codes of injected failures: hipGetErrorString names them (hipstub::INJECTED_A / _B)
    hipErrorStubInjectedB = 9002,
} hipError_t;
typedef enum hipMemcpyKind { hipMemcpyHostToHost = 0, hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2 } hipMemcpyKind;
#define hipStreamNonBlocking 0x01
#define hipHostMallocDefault 0x0

typedef struct hipstub_stream *hipStream_t;
typedef struct hipstub_event *hipEvent_t;

hipError_t hipSetDevice(int device);
hipError_t hipStreamCreateWithFlags(hipStream_t *stream, unsigned flags);
hipError_t hipStreamSynchronize(hipStream_t stream);          // until the FIFO is empty and its last operation has run
hipError_t hipStreamDestroy(hipStream_t stream);              // VIOLATION: the stream still has work
hipError_t hipHostMalloc(void **ptr, size_t size, unsigned flags);      // malloc(size) exactly: AddressSanitizer sees an overrun by one byte
hipError_t hipHostFree(void *ptr);                            // aborts with a message for a pointer hipHostMalloc did not hand out
hipError_t hipEventCreate(hipEvent_t *event);
hipError_t hipEventDestroy(hipEvent_t event);                 // VIOLATION: the event is still pending
hipError_t hipEventRecord(hipEvent_t event, hipStream_t stream);        // VIOLATION: the event is still pending from an earlier record
hipError_t hipEventSynchronize(hipEvent_t event);             // until the operations in front of the record have run
hipError_t hipEventElapsedTime(float *ms, hipEvent_t start, hipEvent_t stop);      // VIOLATION: never recorded / not completed
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t n, hipMemcpyKind kind, hipStream_t stream);
const char *hipGetErrorString(hipError_t e);

// ---- what the test program sets and reads ----
namespace hipstub {
extern const char *const INJECTED_A;      // hipGetErrorString(hipErrorStubInjectedA)
extern const char *const INJECTED_B;
// back to the start: no delays, no injected failures, call counts and violations zero (live objects stay counted)
void reset();
// every operation of a stream waits 0 .. max_us microseconds (seeded) before it runs: the schedule varies, reproducibly per seed
void set_delay(uint64_t seed, unsigned max_us);
// the nth call from now (1 = the next one) fails with `code`; 0 = none.  A failing hipMemcpyAsync enqueues nothing.  A failing
// hipEventSynchronize still waits for the event and then reports the failure.  What is under test is that the report reaches the
// caller and that nothing blocks; the engine treats a slice whose wait failed as arrived (its bytes go to the file, the run fails
// with NS_EHIP), so a wait that returned early would only add a race between the stub's late copy and that write.
void fail_memcpy_at(uint64_t nth, hipError_t code);
void fail_event_sync_at(uint64_t nth, hipError_t code);
void fail_host_malloc_at(uint64_t nth);            // hipErrorOutOfMemory, *ptr = nullptr
void fail_stream_create(bool on);                  // hipErrorOutOfMemory, *stream untouched
// while on, no stream takes an operation off its FIFO (a stream that is being destroyed still runs what it holds): what is
// enqueued stays pending for as long as the test program wants
void hold_streams(bool on);
void quiet(bool on);                               // count violations without printing them (the test of the stub itself)
uint64_t memcpy_calls();                           // since reset(), the failed ones included
uint64_t memcpy_bytes();                           // of the copies that were enqueued
uint64_t event_sync_calls();
uint64_t violations();
const char *first_violation();                     // "" if none
long live_host_allocs();                           // handed out and not freed / destroyed: a leak check that needs no sanitizer
long live_streams();
long live_events();
}
