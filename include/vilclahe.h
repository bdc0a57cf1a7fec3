/* vilclahe.h -- C-ABI of the contrast-limited adaptive histogram equalisation (CLAHE) in front of mVIL-Fusion's feature tracker: a raw
 * 8-bit camera image in, the equalised image out -- or, on the fused path, straight into level 0 of the resident tracker's next forw
 * slot (viltrack.h), whose pyramid is built from it in the same submission.
 *
 * Replaces, inside FeatureTracker::readImage (feature_tracker_/src/feature_tracker.cpp:87-93, equalize: 1 in both shipped configurations):
 * cv::createCLAHE(3.0, cv::Size(8, 8))->apply(_img, img).  The stereo branch (feature_tracker_node.cpp:101) uses OpenCV's defaults 8, 8, 40.0.
 *
 * OpenCV is neither on the machines this was written on nor in the reference tree, so this is a RESTATEMENT WITH A WRITTEN CONTRACT, as
 * viltrack.h is.  It follows OpenCV 4.x modules/imgproc/src/clahe.cpp as its author knows it; NOTHING HERE IS CHECKED AGAINST OpenCV's
 * BITS.  Histogram, clip, redistribution and prefix sum are integer work, exact in any order; the only floating point is a four-term f32
 * blend per pixel in a fixed order, so the device equals tests/clahe_ref.py bit for bit.
 *
 * OUT OF SCOPE: 16-bit images.  The rest of readImage after the equalisation is not here but in vilfeat.h: vfeat_read_image runs these
 * kernels (cfg.equalize) in front of tracking, rejection, detection and the bookkeeping, in one call.
 *
 * ARITHMETIC CONTRACT.  f32 is unfused IEEE float32 in the order written; everything else is integer.  r101 is the one of viltrack.h.
 * W, H the image, tiles_x, tiles_y, clip_limit the configuration.
 *   1 extension   When W % tiles_x == 0 && H % tiles_y == 0 the extended image is the image itself.  Otherwise it is the image padded on the
 *                 right by tiles_x - W % tiles_x columns AND at the bottom by tiles_y - H % tiles_y rows, through r101: as OpenCV, both
 *                 sides are padded whenever either is not divisible, so a divisible side gets a full `tiles` worth of padding.
 *                 tw = We / tiles_x, th = He / tiles_y, area = tw * th.  The padded image is never materialised.
 *   2 constants   (host) clip = 0 when clip_limit == 0, else max((int)(clip_limit * area / 256), 1), the product and quotient in double; a
 *                 value of area or more is held as area (no bin exceeds area, so nothing differs).  lut_scale = 255.0f / (float)area,
 *                 inv_tw = 1.0f / (float)tw, inv_th = 1.0f / (float)th.
 *   3 per tile    hist[256] over the tile's area pixels of the extended image.  With clip > 0: clipped = sum max(hist[i] - clip, 0);
 *                 hist[i] = min(hist[i], clip); batch = clipped / 256, residual = clipped - 256 * batch; hist[i] += batch.  With residual > 0:
 *                 step = max(256 / residual, 1); bin i gets +1 iff i % step == 0 && i / step < residual -- the closed form of OpenCV's
 *                 loop for (i = 0; i < 256 && residual > 0; i += step, residual--); residual * step <= 256, so all of it is handed out.
 *                 lut[i] = sat_u8(rintf((float)(hist[0] + .. + hist[i]) * lut_scale)), rint half-even.
 *   4 per pixel   (x, y) of the ORIGINAL image, v = I(x, y): txf = (float)x * inv_tw - 0.5f, tx1 = floorf(txf), xa = txf - (float)tx1,
 *                 xa1 = 1.0f - xa; then tx2 = min(tx1 + 1, tiles_x - 1), tx1 = max(tx1, 0).  ty1, ty2, ya, ya1 the same from y and inv_th.
 *                 With L[ty][tx] the LUT of tile (tx, ty):
 *                 res = (L[ty1][tx1][v] * xa1 + L[ty1][tx2][v] * xa) * ya1 + (L[ty2][tx1][v] * xa1 + L[ty2][tx2][v] * xa) * ya;
 *                 out = sat_u8(rintf(res)).
 * Plain C, POD only, host pointers.  Needs a HIP device; there is no CPU fallback. */
#ifndef VILCLAHE_H
#define VILCLAHE_H
#include <stdint.h>
#include "vilsolve.h"
#include "viltrack.h"
#ifdef __cplusplus
extern "C" {
#endif

#define VCLAHE_NUM_KERNELS 3         /* k_clahe_hist, k_clahe_lut, k_clahe_blend */
#define VCLAHE_MAX_TILES 16          /* per side */

/* what vclahe_debug_read returns */
enum { VCLAHE_DBG_HIST = 0, VCLAHE_DBG_LUT = 1 };

typedef struct vclahe_ctx vclahe_ctx;

typedef struct vclahe_cfg {
    int32_t width, height;       /* 16 .. 16384 each */
    int32_t tiles_x, tiles_y;    /* 1 .. VCLAHE_MAX_TILES each; reference: 8, 8 */
    double clip_limit;           /* finite, >= 0; 0: no clipping; reference: 3.0 (stereo branch: 40.0) */
} vclahe_cfg;

/* All device and pinned memory is allocated here.  VIL_ERR_INVALID_ARGUMENT for a NULL pointer or a field outside the ranges above, then
 * VIL_ERR_DEVICE without a HIP device. */
int vclahe_create(int32_t device, const vclahe_cfg* cfg, vclahe_ctx** out);
void vclahe_destroy(vclahe_ctx* ctx);
/* Stand-alone.  gray: height rows of width bytes, row_stride bytes apart; out: the same, out_stride apart.  One upload, one clear, three
 * launches, one read-back.  VIL_ERR_INVALID_ARGUMENT for a NULL pointer or a stride < width; nothing is written then. */
int vclahe_apply(vclahe_ctx* ctx, const uint8_t* gray, int32_t row_stride, uint8_t* out, int32_t out_stride);
/* The fused path.  Leaves `tracker` in exactly the state vtrack_push_image(tracker, E, width) would, E being the equalised image (step 4):
 * the slot, cur = forw on the first image, the image count, every pyramid level, the tracker's profile.  The three launches write E into
 * level 0 of the tracker's next forw slot and go into the TRACKER's stream in front of its k_track_pyr launches: one upload, one
 * submission, no host synchronisation in between and no round trip of E.  out != NULL additionally reads E back (out_stride >= width).
 * VIL_ERR_INVALID_ARGUMENT for a NULL ctx, tracker or gray, a tracker of another width, height or device, row_stride < width, or out with
 * out_stride < width; the tracker and `out` stay as they were. */
int vclahe_push(vclahe_ctx* ctx, vtrack_ctx* tracker, const uint8_t* gray, int32_t row_stride, uint8_t* out_or_null, int32_t out_stride);
/* test hook, of the last vclahe_apply / vclahe_push.  VCLAHE_DBG_HIST: the tiles' histograms after clipping and redistribution,
 * [tiles_y][tiles_x][256] int32; VCLAHE_DBG_LUT: their LUTs, [tiles_y][tiles_x][256] bytes.  VIL_ERR_INVALID_ARGUMENT before the first
 * call or when capacity_bytes is too small. */
int vclahe_debug_read(vclahe_ctx* ctx, int32_t what, void* dst, int64_t capacity_bytes);
/* measurement hook, as vtrack_profile_*: HIP events around the kernels; read returns the launch counts and total durations of the
 * VCLAHE_NUM_KERNELS kernels in the order listed above and resets them */
int vclahe_profile_enable(vclahe_ctx* ctx, int32_t enable);
int vclahe_profile_read(vclahe_ctx* ctx, int64_t* launches3, double* total_ms3);

#ifdef __cplusplus
}
#endif
#endif
