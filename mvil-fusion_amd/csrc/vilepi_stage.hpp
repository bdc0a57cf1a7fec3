// vilepi_stage.hpp -- the stages of the epipolar row (vilepi.hip) on device pointers and a stream, enqueue only, for a row that keeps the
// points resident (vilfeat.hip).  vepi_reject and vepi_undistort are callers of the same stages.  csrc-internal, C++ linkage, hidden:
// libvilsolve.so exports nothing from here.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/vilepi.h"

namespace vilepi_stage {

// the context's scratch in its device arena: step 2's points, and per hypothesis the sample, the count, the margin, F and the inlier row
// (`words` 64-bit words apart)
struct Buffers {
    float2 *p1, *p2;
    int *samples, *counts;
    double *margins, *F;
    unsigned long long* bits;
    int words;
};
__attribute__((visibility("hidden"))) Buffers buffers(const vepi_ctx* c);

// Every launch covers n_max points; with d_n not NULL the kernels read the count from *d_n (<= n_max) and the surplus threads exit.
// steps 1-2: cur, forw -> p1, p2
__attribute__((visibility("hidden"))) void lift(const vepi_ctx* c, hipStream_t stream, int n_max, const int* d_n, const float2* cur, const float2* forw, float2* p1, float2* p2);
// steps 3-5 for hypotheses h0 .. h0 + B - 1 of `seed`.  A count below 8 read from *d_n ends every workgroup at once: nothing is written.
// counts (one int per hypothesis) and bits (the inlier rows) may lie in device or in pinned host memory.
__attribute__((visibility("hidden"))) void hypotheses(const vepi_ctx* c, hipStream_t stream, int n_max, const int* d_n, int h0, int B, uint64_t seed, double thr2,
                                                      const Buffers& b, int* counts, unsigned long long* bits);
// step 8 against the table (prev_ids, prev_un) of n_prev entries; (new_ids, new_un) is the table that replaces it
__attribute__((visibility("hidden"))) void undistort(const vepi_ctx* c, hipStream_t stream, int n_max, const int* d_n, const float2* xy, const int* ids, double dt, int n_prev,
                                                     const int* prev_ids, const float2* prev_un, int* new_ids, float2* new_un, float2* un_out, float2* vel_out);
// step 6's N: on the host, in double with the C library's log / pow
__attribute__((visibility("hidden"))) int update_iters(double confidence, double outlier_ratio, int max_iters);

}  // namespace vilepi_stage
