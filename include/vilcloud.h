/* vilcloud.h -- C-ABI of the feature tracker's accumulated depth cloud, resident on the device, and of an exact
 * pcl::ApproximateVoxelGrid as a stand-alone call.
 *
 * Replaces lidar_callback (feature_tracker_/src/feature_tracker_node.cpp:252-337) from the down-sampling of the raw scan to the
 * finished depthCloud that DepthRegister::get_depth reads: per accepted scan the raw points and one 3 x 4 matrix go up, seven counts
 * come back, and vcloud_publish hands the cloud to a vdepth_ctx (vildepth.h) without leaving the device.
 *
 * STAYS ON THE HOST (out of scope here): the `% 2` gate on the scan counter (:254-256), the tf lookup (:259-269), pcl::getTransformation
 * (:270-276) -- the caller builds lidar_to_world in float, exactly as the reference builds transNow, and hands over its upper three rows,
 * row-major, as vdepth_register is given its matrices -- and pcl::fromROSMsg (:279-280).  Points are float [x y z intensity]; the other
 * point types and downsample_all_data_ = false are not covered.
 *
 * A RESTATEMENT WITH A WRITTEN CONTRACT.  PCL is neither available to this project's tests nor part of the reference tree.  Filter A below
 * is written from approximate_voxel_grid.hpp as published in PCL 1.8 - 1.12; it is checked against a sequential restatement of THIS text
 * (tests/cloud_ref.py), bit for bit, and NOT against PCL's bits.
 *
 * ARITHMETIC CONTRACT.  Unfused IEEE float32 in the order written.  p = [x y z intensity].
 *
 * FILTER A(leaf, H): ApproximateVoxelGrid::applyFilter with downsample_all_data_ = true and a table of H entries (PCL's histsize_ is
 * 512).  H is a power of two, 1 <= H <= VCLOUD_MAX_HIST.  Every table entry starts with count 0 and a zero centroid.
 *   1 inv = 1.0f / leaf, leaf a float.
 *   2 per point, in input order: ix = (int)floorf(x * inv), iy and iz likewise; h = (uint32)(ix * 7171 + iy * 3079 + iz * 4231) & (H - 1),
 *     the products and the sum in 32-bit wrap-around arithmetic.
 *   3 if entry h holds a DIFFERENT voxel (ix, iy, iz) and its count is not 0, the entry is flushed first: centroid[k] / (float)count for
 *     all four components, by true division, goes to the next output position; the entry is cleared to zero.
 *   4 the point is added to entry h: four float additions, centroid[k] = centroid[k] + p[k] (the first addition of a run is 0.0f + p[k],
 *     which turns -0 into +0), and the count goes up by one.
 *   5 after the last point every entry with a count is flushed, in the order of the entries.
 *   DEVIATION: a point with a non-finite x, y or z, or for which floorf(c * inv) of a coordinate c lies outside [-2^31, 2^31), is dropped
 *   before step 2 (the reference casts it to int, which is undefined).  The intensity is not looked at: a NaN there is carried through.
 *   The result depends on H and on the order of the points, as PCL's does; it does not depend on anything else.
 *
 * ACCUMULATION, one vcloud_push_scan per accepted scan:
 *   1 A(leaf_scan = 0.2f, H) on the raw scan (:283-288).
 *   2 view filter on the centroids, in order (:292-299).  `abs(p.x > 25)` is the absolute value of a COMPARISON: the point is skipped when
 *     x > max_coord || y > max_coord || z > max_coord, there is no lower bound.  It is then kept iff x >= 0 && fabsf(y / x) <= max_ratio
 *     && fabsf(z / x) <= max_ratio.  With x = 0 a quotient is infinite or NaN, a comparison fails, and the point is dropped -- NOT as in
 *     vildepth.h step 2, whose condition is written the other way round and lets the NaN of 0 / 0 pass.
 *   3 transform (:304) per row of lidar_to_world m: ((m0*x + m1*y) + m2*z) + m3, the form of vildepth.h step 1; the intensity is
 *     unchanged, the order is kept.
 *   4 queue (:307-323): push (stamp, scan); then pop from the front while stamp - front_stamp > window_s, in double, strict: a scan
 *     exactly window_s old stays.
 *   5 fuse (:327-329): the live scans concatenated, oldest first.
 *   6 A(leaf_cloud = 0.1f, H) on the fused cloud (:332-336): the depth cloud.
 *
 * Plain C, POD only, host pointers.  Status codes are those of vilsolve.h.  Needs a HIP device; there is no CPU fallback. */
#ifndef VILCLOUD_H
#define VILCLOUD_H
#include <stdint.h>
#include "vildepth.h"
#include "vilsolve.h"
#ifdef __cplusplus
extern "C" {
#endif

#define VCLOUD_NUM_KERNELS 10
#define VCLOUD_MAX_HIST 2048     /* largest table of filter A */
#define VCLOUD_MAX_SCANS 256     /* largest queue */
/* stages of vcloud_debug_read */
#define VCLOUD_DBG_SCAN_DS 0     /* step 1: the down-sampled scan, sensor frame */
#define VCLOUD_DBG_SCAN_WORLD 1  /* steps 2-3: what went into the queue */
#define VCLOUD_DBG_FUSED 2       /* step 5 */

typedef struct vcloud_ctx vcloud_ctx;

typedef struct vcloud_options {
    float leaf_scan;             /* 0.2f */
    float leaf_cloud;            /* 0.1f */
    int32_t hist_size;           /* 512 */
    float max_coord;             /* 25 */
    float max_ratio;             /* 10 */
    int32_t reserved;
    double window_s;             /* 5.0 */
} vcloud_options;

typedef struct vcloud_summary {
    int32_t n_raw;               /* points handed over */
    int32_t n_scan_ds;           /* after step 1 */
    int32_t n_in_view;           /* after step 2: the points of the scan in the queue */
    int32_t n_scans;             /* scans in the queue after step 4 */
    int32_t n_popped;            /* scans step 4 removed */
    int32_t n_fused;             /* points of step 5 */
    int32_t n_cloud;             /* points of the depth cloud */
} vcloud_summary;

/* All device and pinned memory is allocated here: a queue of max_scans scans of max_scan_points points each, and a fused buffer of
 * max_scans * max_scan_points points.  VIL_ERR_DEVICE without a HIP device, VIL_ERR_INVALID_ARGUMENT for a size < 1, max_scans >
 * VCLOUD_MAX_SCANS or more than 2^27 points in all. */
int vcloud_create(int32_t device, int32_t max_scan_points, int32_t max_scans, vcloud_ctx** out);
void vcloud_destroy(vcloud_ctx* ctx);
/* empty queue, no cloud */
int vcloud_reset(vcloud_ctx* ctx);
void vcloud_default_options(vcloud_options* opts);
/* Filter A alone: n points in, *n_out centroids out in emission order.  n <= max_scans * max_scan_points.  Neither the queue nor the depth
 * cloud nor the stages of vcloud_debug_read are touched.  VIL_ERR_INVALID_ARGUMENT for a leaf that is not a positive finite float, a
 * hist_size that is no power of two in [1, VCLOUD_MAX_HIST], or a capacity (in points) below *n_out, which is still set then. */
int vcloud_filter(vcloud_ctx* ctx, int32_t n, const float* xyzi, float leaf, int32_t hist_size, float* out_xyzi, int32_t capacity, int32_t* n_out);
/* Steps 1-6 as one submission on the context's stream: the raw scan and the matrix go up, the kernels read every point count from a
 * header on the device, and the one host wait at the end brings that header back.  opts may be NULL (the defaults); `out` may be NULL.
 * VIL_ERR_INVALID_ARGUMENT for n > max_scan_points, a non-finite stamp or matrix entry, or options that vcloud_filter would refuse;
 * VIL_ERR_CAPACITY when max_scans scans would still be in the queue after step 4's pop (decided from the stamps alone, before any
 * device work).  The queue, the depth cloud and the debug stages are untouched by a refused call. */
int vcloud_push_scan(vcloud_ctx* ctx, double stamp, const float* lidar_to_world, int32_t n, const float* xyzi, const vcloud_options* opts, vcloud_summary* out);
/* the depth cloud, for tests and logging.  VIL_ERR_INVALID_ARGUMENT when capacity (in points) is below *n, which is still set then. */
int vcloud_read_cloud(vcloud_ctx* ctx, float* out_xyzi, int32_t capacity, int32_t* n);
/* Makes the depth cloud the resident cloud of `depth`, device to device: the effect is that of vdepth_set_cloud with the same points.
 * VIL_ERR_CAPACITY when the cloud has more points than that context's max_cloud_points, VIL_ERR_INVALID_ARGUMENT when it lives on
 * another device; its cloud is kept then. */
int vcloud_publish(vcloud_ctx* ctx, vdepth_ctx* depth);
/* test hook: one of the VCLOUD_DBG_* stages of the last vcloud_push_scan (nothing before the first one and after vcloud_reset) */
int vcloud_debug_read(vcloud_ctx* ctx, int32_t stage, float* out_xyzi, int32_t capacity, int32_t* n);
/* measurement hook, as vdepth_profile_*: HIP events on the context's stream around the launches; read returns the launch counts and total
 * durations of {k_cloud_keys, k_cloud_count, k_cloud_scan, k_cloud_scatter, k_cloud_runs, k_cloud_buckets, k_cloud_emit, k_cloud_view,
 * k_cloud_place, k_cloud_fuse} and resets them */
int vcloud_profile_enable(vcloud_ctx* ctx, int32_t enable);
int vcloud_profile_read(vcloud_ctx* ctx, int64_t* launches10, double* total_ms10);

#ifdef __cplusplus
}
#endif
#endif
