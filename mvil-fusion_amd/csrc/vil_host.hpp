// vil_host.hpp -- the host scaffold shared by the row libraries (vilmap.hip, vilvgicp.hip, vilpreint.hip, vilscan.hip, vildepth.hip,
// vilsc.hip, villoop.hip, vilpgo.hip, vilgmap.hip, viltrack.hip, vilepi.hip, vilclahe.hip, vilfeat.hip, vilcloud.hip, vilfront.hip, villmap.hip; through vil_voxmap.hpp and vil_knn.hpp
// also their headers) and, through vil_comm.hpp and vil_resident.hpp, by the solver itself (vilsolve.hip, vilwindow.hip, vilcomm.hip): one check macro, the
// arena layout, the owner of a row's stream / arena / pinned buffers, the kernel-event profilers, the grow-only buffer (Grown), the mapped pinned record
// (Mapped), the poll of a word in it (await_word) and the event behind a staging copy (Fence).  Everything the solver's context allocates is one of these.
// Header-only, internal linkage or hidden: libvilsolve.so exports nothing from here.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/vilsolve.h"

// a failed HIP call ends the entry point with VIL_ERR_DEVICE; VIL_DEBUG=1 says which call it was
#define VILCHK(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) { if (getenv("VIL_DEBUG")) fprintf(stderr, "%s:%d: %s\n", __FILE_NAME__, __LINE__, hipGetErrorString(e_)); return VIL_ERR_DEVICE; } } while (0)

namespace vilhost {

// A grow-only buffer of T on the device (PINNED, Grown<T, true>: in pinned host memory): the one owner of everything a row allocates on demand.
// reserve(n, alloc) does nothing while n elements fit; otherwise it releases the buffer and allocates alloc >= n elements -- the head
// room is the call site's -- WITHOUT keeping the contents, and is left empty when that fails.  Move-only; frees in its destructor.
template <class T, bool PINNED = false>
struct __attribute__((visibility("hidden"))) Grown {
    T* p = nullptr; size_t cap = 0;                         // cap: elements
    Grown() = default;
    Grown(Grown&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
    Grown& operator=(Grown&& o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }      // (what this held goes with o)
    ~Grown() { release(); }
    hipError_t reserve(size_t n, size_t alloc) {
        if (n <= cap) return hipSuccess;
        release();
        const hipError_t e = PINNED ? hipHostMalloc((void**)&p, alloc * sizeof(T), hipHostMallocDefault) : hipMalloc((void**)&p, alloc * sizeof(T));
        if (e == hipSuccess) cap = alloc; else p = nullptr;
        return e;
    }
    void release() { if (p) { if (PINNED) hipHostFree(p); else hipFree(p); } p = nullptr; cap = 0; }
};

// A zeroed record in pinned host memory that a kernel writes through the device's own pointer to it (a result and the word that
// await_word polls): open() gives both pointers or neither.
struct __attribute__((visibility("hidden"))) Mapped {
    char* h = nullptr; void* d = nullptr;
    Mapped() = default;
    Mapped(const Mapped&) = delete; Mapped& operator=(const Mapped&) = delete;
    ~Mapped() { release(); }
    hipError_t open(size_t bytes) {
        release();
        hipError_t e = hipHostMalloc((void**)&h, bytes, hipHostMallocMapped);
        if (e != hipSuccess) { h = nullptr; return e; }
        memset(h, 0, bytes);
        if ((e = hipHostGetDevicePointer(&d, h, 0)) != hipSuccess) release();
        return e;
    }
    void release() { if (h) hipHostFree(h); h = nullptr; d = nullptr; }
};

// An event that says a stream has passed a point (an asynchronous copy has left its pinned block): created on the first record(),
// wait() blocks the host only while a record() is outstanding.  Both return the HIP error for the caller's check, like Profiler::mark.
struct __attribute__((visibility("hidden"))) Fence {
    hipEvent_t ev = nullptr; bool pending = false;         // (ev: for a hipStreamWaitEvent of the caller's)
    Fence() = default;
    Fence(const Fence&) = delete; Fence& operator=(const Fence&) = delete;
    ~Fence() { if (ev) hipEventDestroy(ev); }
    hipError_t wait() {
        const hipError_t e = pending ? hipEventSynchronize(ev) : hipSuccess;
        if (e == hipSuccess) pending = false;
        return e;
    }
    hipError_t record(hipStream_t stream) {
        hipError_t e = ev ? hipSuccess : hipEventCreateWithFlags(&ev, hipEventDisableTiming);
        if (e == hipSuccess && (e = hipEventRecord(ev, stream)) == hipSuccess) pending = true;
        return e;
    }
};

namespace {

// Spin on a word in pinned memory that a kernel stores last, with system scope; the clock is looked at every 4096 spins.  True: the word
// was seen and what the kernel wrote before it is visible (acquire).  False after limit_ms: the caller falls back to
// hipStreamSynchronize, which surfaces a fault and waits for a device that is merely slow.
inline bool await_word(volatile int* w, int want, int limit_ms) {
    const auto t0 = std::chrono::steady_clock::now();
    for (long spin = 1;; ++spin) {
        if (*w == want) { std::atomic_thread_fence(std::memory_order_acquire); return true; }
        if ((spin & 0xfff) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(limit_ms)) return false;
    }
}

inline size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

// layout of one device arena: every field starts on a 16-byte boundary, in the order it is taken
struct Arena {
    size_t bytes = 0;
    size_t take(size_t n) { const size_t o = bytes; bytes += up16(n); return o; }
};

// kernel times from HIP events: NK kernels, NE events.  A call marks the events around its launches and names, after its
// synchronisation, the (kernel, event, event) spans that were recorded; everything but enable() and read() does nothing while off.
// enable() and mark() return the HIP error: the row puts it through VILCHK, so that the message names the row's line.
template <int NK, int NE>
struct Profiler {
    bool on = false;
    hipEvent_t ev[NE] = {};
    long long n[NK] = {};
    double ms[NK] = {};

    hipError_t enable(int device, bool want) {
        hipError_t err = hipSetDevice(device);
        if (want && !ev[0]) for (hipEvent_t& e : ev) if (err == hipSuccess) err = hipEventCreate(&e);
        if (err == hipSuccess) on = want;
        return err;
    }
    hipError_t mark(int i, hipStream_t stream) { return on ? hipEventRecord(ev[i], stream) : hipSuccess; }
    void span(int kernel, int ev_a, int ev_b) {
        float t = 0.f;
        if (on && hipEventElapsedTime(&t, ev[ev_a], ev[ev_b]) == hipSuccess) { ms[kernel] += t; n[kernel]++; }
    }
    void read(int64_t* launches, double* total_ms) {
        for (int k = 0; k < NK; ++k) { launches[k] = n[k]; total_ms[k] = ms[k]; n[k] = 0; ms[k] = 0.0; }
    }
    void destroy() { for (hipEvent_t e : ev) if (e) hipEventDestroy(e); }
};

// The same for a call whose number of launches is not fixed (vilpgo.hip: an enqueued sequence per iteration): mark() records an event before a
// group of launches of one kernel and grows the pool on demand, collect() -- after the call's synchronisation -- gives the time between
// two marks to the first one's kernel.  kernel < 0 closes the last group.
template <int NK>
struct EventLog {
    struct Mark { int kernel, launches; };
    bool on = false;
    std::vector<hipEvent_t> ev;
    std::vector<Mark> marks;
    long long n[NK] = {};
    double ms[NK] = {};

    hipError_t mark(int kernel, int launches, hipStream_t stream) {
        if (!on) return hipSuccess;
        if (marks.size() == ev.size()) { hipEvent_t e; const hipError_t err = hipEventCreate(&e); if (err != hipSuccess) return err; ev.push_back(e); }
        const hipError_t err = hipEventRecord(ev[marks.size()], stream);
        if (err == hipSuccess) marks.push_back({kernel, launches});
        return err;
    }
    void collect() {
        for (size_t i = 0; i + 1 < marks.size(); ++i) {
            float t = 0.f;
            if (marks[i].kernel >= 0 && hipEventElapsedTime(&t, ev[i], ev[i + 1]) == hipSuccess) { ms[marks[i].kernel] += t; n[marks[i].kernel] += marks[i].launches; }
        }
        marks.clear();
    }
    void read(int64_t* launches, double* total_ms) {
        for (int k = 0; k < NK; ++k) { launches[k] = n[k]; total_ms[k] = ms[k]; n[k] = 0; ms[k] = 0.0; }
    }
    void destroy() { for (hipEvent_t e : ev) hipEventDestroy(e); }
};

inline bool has_device(int dev) {                          // no CPU fallback
    int ndev = 0;
    return hipGetDeviceCount(&ndev) == hipSuccess && dev >= 0 && dev < ndev;
}

// what a row's context owns on its device: the stream, one arena of device memory (none when arena_bytes is 0) and up to four
// pinned host buffers.  The contexts derive from it.  open() and pin() return the HIP error for the row's VILCHK.
// Teardown is close(), which selects the device, then delete: a context's Grown and Mapped members free in their destructors, after
// close(), with the context's device still current.  close() has destroyed the stream by then, which hipFree / hipHostFree do not need.
struct Device {
    int device = -1;                                        // -1: never opened, close() has nothing to free
    hipStream_t stream = nullptr;
    char* d_mem = nullptr;
    void* pinned[4] = {};
    int n_pinned = 0;

    hipError_t open(int dev, size_t arena_bytes) {
        if (!has_device(dev)) return hipErrorInvalidDevice;
        hipError_t err = hipSetDevice(dev);
        if (err != hipSuccess) return err;
        device = dev;
        err = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking);
        if (err == hipSuccess && arena_bytes) err = hipMalloc(&d_mem, arena_bytes);
        return err;
    }
    template <class T>
    hipError_t pin(T** p, size_t bytes) {
        if (n_pinned == 4) return hipErrorOutOfMemory;
        const hipError_t e = hipHostMalloc((void**)p, bytes, hipHostMallocDefault);
        if (e == hipSuccess) pinned[n_pinned++] = *p;
        return e;
    }
    template <class P>
    void close(P& prof) {
        if (device < 0) return;
        hipSetDevice(device);
        hipFree(d_mem);
        for (int i = 0; i < n_pinned; ++i) hipHostFree(pinned[i]);
        prof.destroy();
        if (stream) hipStreamDestroy(stream);
    }
};

}  // namespace
}  // namespace vilhost
