// vilmap_stage.hpp -- the scan-to-map registration of include/vilmap.h (vilmap.hip) for a row that already has the map and the scan on
// the device (villmap.hip).  vmap_set_map and vmap_align run the same two functions with host pointers.  csrc-internal, C++ linkage,
// hidden: libvilsolve.so exports nothing from here.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/vilmap.h"

namespace vilmap_stage {

// vmap_set_map for clouds in memory of the context's device that the caller owns: the same copies (device to device), the same
// grid_build_adaptive, the same wait at the end.  The caller has waited for whatever wrote the clouds.
__attribute__((visibility("hidden"))) int set_map_resident(vmap_ctx* c, int32_t n_corner, const float* d_corner_xyzi, int32_t n_surf, const float* d_surf_xyzi);
// vmap_align for stacks in memory of the context's device: the same gate, the same two rounds, the same kernels and grids.  The caller
// has waited for whatever wrote the stacks; the call ends with vmap_align's own wait.
__attribute__((visibility("hidden"))) int align_resident(vmap_ctx* c, vil_ctx* solver, int32_t n_corner, const float* d_corner_xyzi, int32_t n_surf, const float* d_surf_xyzi,
                                                         double* q_xyzw, double* t, const vil_options* opts, vmap_summary* out);
// The rotation matrix (row-major, 9 doubles) and the translation (3 doubles) that the last solve of the last vmap_align / align_resident
// left on the device, or null when that call ran no one-launch solve (the gate failed, or the window solver took the scan).
__attribute__((visibility("hidden"))) const double* device_pose(vmap_ctx* c);
// the host's quaternion [x y z w] -> rotation matrix (row-major), the one vmap_associate and the first search of vmap_align use
__attribute__((visibility("hidden"))) void quat_to_R(const double* q_xyzw, double* R9);

}  // namespace vilmap_stage
