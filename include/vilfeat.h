/* vilfeat.h -- C-ABI of the device-resident feature tracker of mVIL-Fusion: FeatureTracker::readImage as ONE call, camera image in, the
 * /feature_tracker_/feature message out, the points, ids, track counts and the velocity table resident in between.
 *
 * Replaces the host code that connects the three rows behind viltrack.h, vilepi.h and vilclahe.h (feature_tracker_/src/feature_tracker.cpp:
 * reduceVector :13-29, addPoints :71-79, the two compactions :115-128 and :193-198, cur_pts = forw_pts :160-166, updateID :204-214;
 * feature_tracker_node.cpp: the updateID loop and the message assembly :113-167).  The arithmetic of every step is that of those rows,
 * by their written contracts and by the same kernels; this header adds the bookkeeping between them.
 *
 * OUT OF SCOPE: NUM_OF_CAM > 1 / STEREO_TRACK; the fisheye mask; prev_pts / prev_img (write-only in the reference); the depth channel
 * (vdepth_register takes the message's points); the ROS node with its frequency schedule, the init_pub skip of the first published message
 * and the discontinuity check -- the caller decides `publish` and what to do with the first message.
 *
 * THE CALL.  vfeat_read_image(img, time_s, publish) is readImage(img, time_s) with PUB_THIS_FRAME = publish, then the updateID loop of
 * img_callback, then (publish) the message for NUM_OF_CAM = 1.  Exactly this sequence:
 *   1 image       the image is pushed as vtrack_push_image does, equalised first as vclahe_push does when cfg.equalize.  On the first image
 *                 (and the first after vfeat_reset) cur = forw.
 *   2 LK          with n_before > 0 points: viltrack.h steps 3-6 from cur_pts (status = LK's status AND inBorder), then an ORDERED
 *                 compaction of cur_pts, forw_pts, ids, track_cnt on status.  n_tracked survive.
 *   3 count       track_cnt += 1 for every survivor -- on every image, published or not.
 *   4 rejectWithF only if publish and n_tracked >= 8: vilepi.h steps 1-7 with seed `seed`, thr = cfg.f_threshold, cfg.confidence.  All
 *                 cfg.max_iters hypotheses are evaluated in one launch; step 6's loop runs on the host, in double with the C library's
 *                 log / pow as that contract demands, over the RECORDS of the counts: hypothesis h is a record when count_h > max(7, every
 *                 earlier count).  The loop changes its state at records only, so replaying it over them returns what replaying it over
 *                 all counts returns: the best hypothesis, its count, and consumed = max(niters, h_last + 1) with h_last the last record the
 *                 loop took (max_iters without one).  Then an ordered compaction on the best hypothesis' inlier flags; without a model all
 *                 flags are 1.
 *   5 setMask ... only if publish.  PRIORITY ORDER: track_cnt descending, ties in current order.  (A RESTATEMENT: the reference's std::sort
 *                 is unstable and viltrack.h leaves the order to its caller; this row fixes the stable order.)  Then viltrack.h steps 7-10
 *                 with cfg.min_dist, cfg.quality and max(0, cfg.max_cnt - n_kept) picks; an ordered compaction on `kept`; addPoints: the
 *                 picks appended in pick order with id = -1, track_cnt = 1.
 *   6 roles       cur_pts = forw_pts; the images' roles move as in viltrack.h.
 *   7 undistort   vilepi.h step 8 on all n points with dt = time_s - the previous call's time_s, on the ids BEFORE updateID: a new point
 *                 carries -1 here.  The table that replaces the previous one is keyed the same way.
 *   8 updateID    every id -1 becomes next_id++, in index order.
 *   9 message     if publish: one row per point with track_cnt > 1, in state order: points_xyz = (un.x, un.y, 1.0f), id = (float)id,
 *                 u, v = cur_pts, vx, vy = pts_velocity.
 * QUIRKS of the reference that follow from 7 and 8, kept: a corner has zero velocity on the image where it is detected AND on the next one
 * (the table holds it under -1), so in the second published image of a sequence every velocity is zero.  track_cnt grows on unpublished
 * images; RANSAC, setMask and detection do not run on them.  n <= max_cnt always.
 *
 * BUS AND WAITS.  Per call the image goes up (width * height bytes; everything else is kernel arguments) and the header and the message
 * come down, written by the kernels into pinned host memory: VFEAT_HEADER_BYTES (4 less when step 4's launches are skipped), 8 bytes
 * per record of step 4, 32 bytes per message row.  The points, ids, counts, tables, RANSAC counts and inlier rows never leave the device.  The host waits for the stream at most twice
 * on a published image with n_before >= 8 (after the hypotheses, whose loop is the host's, and at the end), once otherwise.  A stage's
 * point count is read by its kernels from a device header; the launches cover the count before the stage, which only shrinks.
 * Results are bit-identical from run to run and from process to process: every compaction and the ranking are by prefix sums and counting,
 * never by the arrival order of atomics.
 *
 * ERRORS.  VIL_ERR_INVALID_ARGUMENT (a NULL pointer, row_stride < width, publish without msg or with a NULL array in it, NaN time_s):
 * nothing is touched; the next valid call behaves as if the bad one had not happened.  VIL_ERR_UNSUPPORTED (step 9's candidates exceed
 * max_candidates, as vtrack_detect) and VIL_ERR_DEVICE write no output and LEAVE THE CONTEXT AS AFTER vfeat_reset -- the image slot has
 * been flipped by then, and "start again from a first image" is what the node does on a broken stream anyway.
 * Plain C, POD only, host pointers.  Needs a HIP device; there is no CPU fallback. */
#ifndef VILFEAT_H
#define VILFEAT_H
#include <stdint.h>
#include "vilsolve.h"
#include "viltrack.h"
#include "vilepi.h"
#include "vilclahe.h"
#ifdef __cplusplus
extern "C" {
#endif

#define VFEAT_NUM_KERNELS 5          /* k_feat_compact_lk, k_feat_records, k_feat_compact_rank, k_feat_compact_add, k_feat_finish */
#define VFEAT_MIN_POINTS_LIMIT 8
#define VFEAT_MAX_POINTS_LIMIT 4096  /* the rows' limits; a thread of the one-workgroup kernels takes 4 points */
#define VFEAT_HEADER_BYTES 64        /* the header the kernels mirror to the host: 4 bytes after LK, 4 + the records after the hypotheses, 56 at the end */
#define VFEAT_ROW_BYTES 32           /* a message row: 3 + 5 floats */

/* what vfeat_debug_read returns */
enum { VFEAT_DBG_STATE = 0, VFEAT_DBG_UN_VEL = 1, VFEAT_DBG_CUR_LEVEL = 2, VFEAT_DBG_FORW_LEVEL = 3 };

typedef struct vfeat_ctx vfeat_ctx;

typedef struct vfeat_cfg {
    double fx, fy, cx, cy, k1, k2, p1, p2;  /* as vepi_cfg */
    double focal;                           /* as vepi_cfg; reference: 460 */
    double clip_limit;                      /* as vclahe_cfg; ignored when equalize = 0 */
    double f_threshold;                     /* > 0; reference: F_THRESHOLD 1.0 */
    double confidence;                      /* in (0, 1); reference: 0.99 */
    float quality;                          /* in (0, 1]; reference: 0.01 */
    int32_t width, height;                  /* 16 .. 16384 each */
    int32_t max_level;                      /* 0 .. VTRACK_MAX_LEVEL */
    int32_t max_points;                     /* VFEAT_MIN_POINTS_LIMIT .. VFEAT_MAX_POINTS_LIMIT */
    int32_t max_candidates;                 /* >= 1, as vtrack_cfg */
    int32_t model;                          /* VEPI_MODEL_*; PINHOLE only, the others give VIL_ERR_UNSUPPORTED */
    int32_t max_iters;                      /* 1 .. VEPI_MAX_ITERS_LIMIT; reference: 1000 */
    int32_t equalize;                       /* 0 / 1 */
    int32_t tiles_x, tiles_y;               /* 1 .. VCLAHE_MAX_TILES each; ignored when equalize = 0 */
    int32_t max_cnt;                        /* 1 .. max_points; reference: MAX_CNT 150 */
    int32_t min_dist;                       /* 0 .. VTRACK_MAX_MIN_DIST; reference: MIN_DIST 30 */
    int32_t reserved;
} vfeat_cfg;

/* caller-owned host arrays with room for cfg.max_cnt rows (points_xyz: 3 floats per row).  The five channel pointers and a depth array
 * from vdepth_register(.., n_rows, points_xyz, ..) go into vilformat::decode_feature_cloud as they are. */
typedef struct vfeat_msg {
    float* points_xyz;
    float *id, *u, *v, *vx, *vy;
    int32_t n_rows;                         /* written by the call; 0 with publish = 0 */
    int32_t reserved;
} vfeat_msg;

typedef struct vfeat_summary {
    int32_t n_before, n_tracked;            /* points entering LK, survivors of step 2 */
    int32_t n_inliers;                      /* survivors of step 4; n_tracked when RANSAC is skipped or finds nothing */
    int32_t found, best_hypothesis, consumed;   /* as vepi_summary; 0, -1, 0 when RANSAC is skipped */
    int32_t n_records;                      /* records of step 4 the kernels reported */
    int32_t n_kept, n_candidates, n_new;    /* step 5, as vtrack_summary; 0 when unpublished */
    int32_t n;                              /* points now */
    int32_t n_rows;                         /* message rows */
    int32_t next_id;                        /* the id the next new point gets */
    int32_t host_waits;                     /* stream synchronisations of this call */
    int64_t bytes_up, bytes_down;           /* bytes of explicit copies up; bytes the kernels wrote to pinned host memory */
} vfeat_summary;

/* All device and pinned memory is allocated here, the owned contexts of the three rows included.  VIL_ERR_INVALID_ARGUMENT for a NULL
 * pointer or a value outside the ranges above (non-finite included), then VIL_ERR_UNSUPPORTED for another model than PINHOLE, then
 * VIL_ERR_DEVICE without a HIP device. */
int vfeat_create(int32_t device, const vfeat_cfg* cfg, vfeat_ctx** out);
void vfeat_destroy(vfeat_ctx* ctx);
/* gray: height rows of width bytes, row_stride bytes apart.  seed: vepi_reject's seed for this image.  msg may be NULL when publish = 0;
 * summary may be NULL. */
int vfeat_read_image(vfeat_ctx* ctx, const uint8_t* gray, int32_t row_stride, double time_s, int32_t publish, uint64_t seed, vfeat_msg* msg, vfeat_summary* summary);
/* points, images and the velocity table are forgotten: the next image is a first image.  next_id keeps counting. */
int vfeat_reset(vfeat_ctx* ctx);
/* test hook.  _STATE: int32 n, then cur_pts n x 2 f32, ids n i32 (after updateID), track_cnt n i32, packed.  _UN_VEL: cur_un_pts n x 2 f32,
 * then pts_velocity n x 2 f32, of all n points, also after an unpublished image.  _CUR_LEVEL / _FORW_LEVEL: pyramid level `arg` of the owned
 * tracker, as vtrack_debug_read.  VIL_ERR_INVALID_ARGUMENT when capacity_bytes is too small. */
int vfeat_debug_read(vfeat_ctx* ctx, int32_t what, int32_t arg, void* dst, int64_t capacity_bytes);
/* measurement hook, as vtrack_profile_*: HIP events around the NEW kernels of this row (those of the three rows keep their own hooks);
 * read returns the launch counts and total durations of the VFEAT_NUM_KERNELS kernels in the order listed above and resets them */
int vfeat_profile_enable(vfeat_ctx* ctx, int32_t enable);
int vfeat_profile_read(vfeat_ctx* ctx, int64_t* launches5, double* total_ms5);

#ifdef __cplusplus
}
#endif
#endif
