// vilcloud_stage.hpp -- filter A of include/vilcloud.h (vilcloud.hip) for a row that already has the points on the device (vilfront.hip).
// vcloud_filter, vcloud_push_scan and the stage run the same enqueue_filter.  csrc-internal, C++ linkage, hidden: libvilsolve.so exports
// nothing from here.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/vilcloud.h"
#include "vil_host.hpp"

namespace vilcloud_stage {

// what vcloud_filter refuses in a leaf and a table size
__attribute__((visibility("hidden"))) bool accepts(float leaf, int32_t hist_size);
// Filter A(leaf, hist_size), enqueue only, on the context's stream: min(*d_n, n_upper) points of `in`, the centroids in emission order
// to `out` (room for n_upper points), their number to *d_n_out.  in, d_n, out and d_n_out are memory of the context's device that the
// caller owns; n_upper <= the context's max_scans * max_scan_points; leaf and hist_size are ones that accepts() accepts.
// ORDERING, by events and without a host wait: the context's stream first waits for `ready`, which the caller recorded on its own
// stream behind the writes of `in` and *d_n; when everything is enqueued, `done` is recorded on the context's stream, and the caller
// makes its stream (hipStreamWaitEvent on done.ev) or the host (done.wait()) wait for it before it touches out or *d_n_out.
// A VIL_* status; the context's queue, depth cloud and debug stages are not touched, its filter work space is.
__attribute__((visibility("hidden"))) int filter_resident(vcloud_ctx* c, const float4* in, const int* d_n, int n_upper, float leaf, int32_t hist_size, float4* out, int* d_n_out,
                                                          hipEvent_t ready, vilhost::Fence& done);

}  // namespace vilcloud_stage
