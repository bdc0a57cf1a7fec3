// viltrack_stage.hpp -- the two stages of vtrack_push_image (viltrack.hip), for a row that produces the image on the device instead of
// uploading it (vilclahe.hip).  csrc-internal, C++ linkage, hidden: libvilsolve.so exports nothing from here.
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

// Stage 1, "stage the image into level 0 of the next slot", is the caller's: it enqueues on t.stream whatever writes t.level0.
// target() changes nothing in the tracker.
__attribute__((visibility("hidden"))) Target target(const vtrack_ctx* c);
// Stage 2: build the pyramid from level 0 on the same stream, synchronise, flip the slots, account the profile.  A VIL_* status; the
// slots are flipped only on VIL_OK.
__attribute__((visibility("hidden"))) int finish_push(vtrack_ctx* c);

}  // namespace viltrack_stage
