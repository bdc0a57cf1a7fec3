// villoop_stage.hpp -- the hand-over of clouds to a fitness context (villoop.hip) for a row that already has the points on the device
// (vilfront.hip).  vloop_set_source and vloop_set_target are callers of the same stages.  csrc-internal, C++ linkage, hidden:
// libvilsolve.so exports nothing from here.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/villoop.h"

namespace villoop_stage {

// Replaces the resident source by 1 <= n <= max_points FINITE points (float xyz, stride 3) at src: the copy (`kind`: from host memory,
// staged through the context's pinned buffer, or from memory of the same device WHOSE WRITES ARE COMPLETE -- ordering by a wait, not
// by an event) on the context's stream, and the wait for it: src may be overwritten when this returns.  A VIL_* status; there is no
// resident source when it is not VIL_OK.
__attribute__((visibility("hidden"))) int install_source(vloop_ctx* c, int32_t n, const float* src, hipMemcpyKind kind);
// The resident source becomes the target, device to device on the context's stream, with the search grid rebuilt (build_grid) when
// the cloud has at least the points vloop_set_grid asks for, exactly as vloop_set_target does; the source stays resident.
// VIL_ERR_INVALID_ARGUMENT without a source; there is no resident target after any other failure.
__attribute__((visibility("hidden"))) int promote_source(vloop_ctx* c);

}  // namespace villoop_stage
