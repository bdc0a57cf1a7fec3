// vilclahe_stage.hpp -- the two stages of a CLAHE submission (vilclahe.hip) for a row that owns the upload and the stream (vilfeat.hip).
// vclahe_apply and vclahe_push are callers of the same stages.  csrc-internal, C++ linkage, hidden: libvilsolve.so exports nothing from here.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/vilclahe.h"

namespace vilclahe_stage {

// the raw image packed into the context's pinned buffer (W x H bytes) and where the kernels read it on the device
struct Staged {
    const uint8_t* host;
    uint8_t* dev;
};
// Stage 1: pack the rows.  The caller enqueues the copy host -> dev on its stream.
__attribute__((visibility("hidden"))) Staged stage_image(vclahe_ctx* c, const uint8_t* gray, int row_stride);
// Stage 2, enqueue only: the clear of the histograms and the three launches on `stream`; the equalised image goes to dst and, when not
// NULL, to dst2 (W x H bytes, rows W apart).  A VIL_* status.
__attribute__((visibility("hidden"))) int enqueue_kernels(vclahe_ctx* c, hipStream_t stream, uint8_t* dst, uint8_t* dst2);

}  // namespace vilclahe_stage
