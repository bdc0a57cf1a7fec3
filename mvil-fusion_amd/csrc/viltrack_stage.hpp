// viltrack_stage.hpp -- the stages of the tracker row (viltrack.hip) for the rows that drive it from the device side: vilclahe.hip produces
// the image on the device instead of uploading it, vilfeat.hip chains push, LK and detection without a host step in between.  The extern "C"
// entry points of viltrack.hip are callers of the same stages.  csrc-internal, C++ linkage, hidden: libvilsolve.so exports nothing from here.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/viltrack.h"

namespace viltrack_stage {

// where the next image goes: level 0 of the slot that becomes forw (W x H bytes, rows W apart), and the stream the tracker's launches go to
struct Target {
    uint8_t* level0;
    hipStream_t stream;
    int device, width, height;
};

// counters of one detection (ints) in the tracker's arena, in front of kept and new_xy
enum { H_NKEPT = 0, H_MAXBITS, H_NCAND, H_NPICK, H_NNEW, H_ROUNDS, H_FAIL, H_INTS = 16 };
// what a detection leaves in the tracker's arena (device pointers): the counters, setMask's decisions, the picks in rank order
struct Detection {
    int* hdr;
    uint8_t* kept;
    float* new_xy;
};

// Stage 1, "stage the image into level 0 of the next slot", is the caller's: it enqueues on t.stream whatever writes t.level0.
// target() changes nothing in the tracker.  stage_image() packs the rows of a host image into the tracker's pinned buffer (W x H bytes)
// for a caller that uploads it.
__attribute__((visibility("hidden"))) Target target(const vtrack_ctx* c);
__attribute__((visibility("hidden"))) const uint8_t* stage_image(vtrack_ctx* c, const uint8_t* gray, int row_stride);
// Stage 2, enqueue only: the pyramid from level 0 on the tracker's stream.  commit_push() flips the slots (host state only); a caller
// that enqueues more work on the same stream may commit at once.  finish_push() is the two with the synchronisation and the profile
// between them: a VIL_* status, the slots are flipped only on VIL_OK.  forget() drops both images: the next push is a first image.
__attribute__((visibility("hidden"))) int enqueue_push(vtrack_ctx* c);
__attribute__((visibility("hidden"))) void commit_push(vtrack_ctx* c);
__attribute__((visibility("hidden"))) int finish_push(vtrack_ctx* c);
__attribute__((visibility("hidden"))) void forget(vtrack_ctx* c);

// Steps 3-6 and 7-10 on device pointers, enqueue only, on the tracker's stream.  The launches cover n_max points; with d_n not NULL the
// kernels read the count from *d_n (<= n_max) and the surplus workgroups exit.  d_pts, d_forw: [x y] floats; d_status: bytes.
__attribute__((visibility("hidden"))) int enqueue_lk(vtrack_ctx* c, int n_max, const int* d_n, const float* d_pts, float* d_forw, uint8_t* d_status);
__attribute__((visibility("hidden"))) int enqueue_detect(vtrack_ctx* c, int n_max, const int* d_n, const float* d_tracks, int min_dist, int max_cnt, float quality, Detection* out);

}  // namespace viltrack_stage
