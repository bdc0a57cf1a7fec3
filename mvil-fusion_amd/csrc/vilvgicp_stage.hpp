// vilvgicp_stage.hpp -- the hand-over of a source cloud to a registration context (vilvgicp.hip) for a row that already has the points
// on the device (vilfront.hip).  vgicp_set_source is a caller of the same stage.  The other half of the exchange, the source becoming the
// target, is public: vgicp_promote_source.  csrc-internal, C++ linkage, hidden: libvilsolve.so exports nothing from here.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/vilvgicp.h"

namespace vilvgicp_stage {

// what vgicp_align refuses in its options
__attribute__((visibility("hidden"))) bool accepts(const vgicp_options& o);
// Replaces the resident source by n >= 1 points (float xyz, stride 3) at src.  kind = hipMemcpyHostToDevice: src is host memory, cov9
// (n x 9 doubles, host) may be given, as in vgicp_set_source.  kind = hipMemcpyDeviceToDevice: src is memory of the context's device
// WHOSE WRITES ARE COMPLETE (the caller has waited for them: ordering by a wait, not by an event), cov9 is NULL, the copy is enqueued on
// the context's stream.  Without cov9 the covariances are estimated on the device from the KNN_MAX = 20 nearest neighbours, and the
// host wait that ends that estimate also ends the copy: src may be overwritten when this returns.
// A VIL_* status; there is no resident source when it is not VIL_OK.
__attribute__((visibility("hidden"))) int install_source(vgicp_ctx* c, int32_t n, const float* src, const double* cov9, hipMemcpyKind kind);

}  // namespace vilvgicp_stage
