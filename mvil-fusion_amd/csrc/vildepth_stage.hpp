// vildepth_stage.hpp -- the hand-over of a cloud to a depth context (vildepth.hip) for a row that already has the points on the device
// (vilcloud.hip).  vdepth_set_cloud and vcloud_publish are callers of the same stage.  csrc-internal, C++ linkage, hidden: libvilsolve.so
// exports nothing from here.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/vildepth.h"

namespace vildepth_stage {

// what a caller has to check before it hands a cloud over
struct Target {
    int device;
    int max_cloud_points;
};
__attribute__((visibility("hidden"))) Target target(const vdepth_ctx* c);
// Replaces the resident cloud by n <= max_cloud_points points [x y z intensity] at src: the copy (`kind`: from pinned host memory or from
// memory of the same device whose writes are complete) on the context's stream, the wait for it, then n becomes the cloud's size;
// n = 0 is the "no cloud" state and copies nothing.  A VIL_* status; the resident cloud's size is kept when it is not VIL_OK.
__attribute__((visibility("hidden"))) int replace_cloud(vdepth_ctx* c, int n, const float* src, hipMemcpyKind kind);

}  // namespace vildepth_stage
