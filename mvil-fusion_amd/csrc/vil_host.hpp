// vil_host.hpp -- the host scaffold shared by the row libraries (vilmap.hip, vilvgicp.hip, vilpreint.hip, vilscan.hip, vildepth.hip,
// vilsc.hip, villoop.hip, vilpgo.hip, vilgmap.hip, viltrack.hip, vilepi.hip, vilclahe.hip, vilfeat.hip, vilcloud.hip): one check macro, the arena layout, the owner of a row's stream / arena / pinned buffers and the kernel-event profilers.
// Header-only, internal linkage: libvilsolve.so exports nothing from here.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/vilsolve.h"

// a failed HIP call ends the entry point with VIL_ERR_DEVICE; VIL_DEBUG=1 says which call it was
#define VILCHK(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) { if (getenv("VIL_DEBUG")) fprintf(stderr, "%s:%d: %s\n", __FILE_NAME__, __LINE__, hipGetErrorString(e_)); return VIL_ERR_DEVICE; } } while (0)

namespace vilhost {
namespace {

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
