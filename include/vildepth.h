/* vildepth.h -- C-ABI of the LiDAR depth association of mVIL-Fusion's feature tracker: the accumulated world-frame depth cloud and the
 * undistorted features of one camera image in, one depth per feature out (channel 5 of the feature message, obs8[7] of vilformat.hpp,
 * the "V-L" coupling: FeatureTable turns depth > 0 into lidar_depth_flag and the solve holds that inverse depth constant).
 *
 * Replaces DepthRegister::get_depth (feature_tracker_/src/feature_tracker.h:98-343), called once per camera image at
 * feature_tracker_node.cpp:176.  The cloud stays on the device between calls (the reference replaces it once per accepted LiDAR scan
 * and reads it once per image); per image only two 3 x 4 matrices and the features go up, the depths and four counts come back.
 *
 * STAYS ON THE HOST (out of scope here):
 *   - the two matrices.  world_to_lidar is transNow.inverse() (:122-132: tf pose -> quaternion -> roll / pitch / yaw ->
 *     pcl::getTransformation -> Affine3f inverse), lidar_to_view is Tlc_ * TransFormLC.inverse() (:134-140).  The caller builds both in
 *     float, exactly as the reference does, and hands over the upper three rows, row-major.  mvil-fusion_amd/depthreg.py::view_matrices
 *     builds them from rotations and translations for the tests.
 *   - lidar_callback's accumulation of depthCloud (feature_tracker_node.cpp:252-337: pcl::ApproximateVoxelGrid, the view filter, the
 *     transform to world, the 5 s queue) is no part of THIS header.  It has a device row of its own, vilcloud.h, whose publish call
 *     makes its cloud the resident cloud here without a trip through the host; a caller that builds the cloud itself still uploads it
 *     with the set_cloud call below.
 *
 * ARITHMETIC CONTRACT.  Unfused IEEE float32 in the order written, except where marked double.  p = [x y z intensity].
 *   1 transform   (:132, :140) per row of a matrix m: ((m0*x + m1*y) + m2*z) + m3.  lidar_to_view is applied to the rounded result of
 *                 world_to_lidar; the intensity is carried along unchanged.
 *                 DEVIATION: a point with a non-finite coordinate after either transform is dropped (the reference casts NaN to int
 *                 there, which is undefined).
 *   2 view filter (:150) the point is skipped when x < 0 || fabsf(y / x) > 10 || fabsf(z / x) > 10.  x = 0 behaves as IEEE division
 *                 makes it: with x = 0 and y = 0 the quotient is NaN, the comparison is false, and the point passes, as in the reference.
 *   3 bins        (:153-160) row_angle = float(double(atan2f(z, sqrtf(x*x + y*y))) * 180.0 / M_PI + 90.0), row = int(roundf(row_angle /
 *                 0.5f)); col_angle = float(double(atan2f(x, y)) * 180.0 / M_PI), col = int(roundf(col_angle / 0.5f)); the point is kept
 *                 when row and col both lie in [0, VDEPTH_BINS).  Only atan2f is the device library's.
 *   4 closest     (:162-167) dist = sqrtf((x*x + y*y) + z*z); a bin keeps the point with the smallest dist, the comparison is strict, so
 *                 among equal distances the smallest cloud index wins.  A point with dist >= FLT_MAX never enters (dist < FLT_MAX fails
 *                 in the reference too).  DEVIATION: a point with dist == 0 (exactly at the sensor) is dropped; in the reference it
 *                 becomes a NaN point of the kd-tree's input.
 *   5 emission    (:172-179) occupied bins in row-major order.
 *   6 sphere      (:241-250) x, y and z each divided by range = dist; range is kept as the fourth component.  With fewer than 10 sphere
 *                 points every depth is -1 (:251).
 *   7 feature     (:225-237) n = sqrtf((fx*fx + fy*fy) + fz*fz), v = f / n component-wise, sphere point p = (v.z, -v.x, -v.y).
 *                 DEVIATION: a feature with a non-finite p gets -1 (the reference hands NaN to the kd-tree).
 *   8 3-NN        (:271-272) squared distance (dx*dx + dy*dy) + dz*dz, d = p - neighbour; the three nearest sphere points ordered by
 *                 (distance, sphere index).  pcl / FLANN may order neighbours at EQUAL distance differently; that can change the result
 *                 only through which of several tied third neighbours is taken.  The search is exact.  A feature is accepted when three
 *                 neighbours exist and d2[2] < float(pow(sin(0.5 / 180.0 * M_PI) * 5.0, 2)) (:268, evaluated in double on the host).
 *   9 depth       (:274-339) r1..r3 the ranges in neighbour order; max - min > 2 gives -1; s = ((r1 + r2) + r3) / 3; depth = p.x * s,
 *                 returned only when depth > 3.0, otherwise -1.
 * Results are bit-reproducible against a float32 restatement (tests/depthreg_ref.py) wherever atan2f's last bits do not move a point
 * across a bin edge.
 * Plain C, POD only, host pointers.  Needs a HIP device; there is no CPU fallback. */
#ifndef VILDEPTH_H
#define VILDEPTH_H
#include <stdint.h>
#include "vilsolve.h"
#ifdef __cplusplus
extern "C" {
#endif

#define VDEPTH_BINS 360          /* num_bins: the range image is VDEPTH_BINS x VDEPTH_BINS bins of 0.5 degrees */
#define VDEPTH_NUM_KERNELS 3
#define VDEPTH_MIN_SPHERE 10     /* :251 */

typedef struct vdepth_ctx vdepth_ctx;

typedef struct vdepth_summary {
    int32_t n_cloud;             /* points of the resident cloud */
    int32_t n_in_view;           /* points that reached the range image (steps 1-4) */
    int32_t n_sphere;            /* occupied bins = points of the down-sampled sphere cloud */
    int32_t n_with_depth;        /* features whose depth_out is not -1 */
} vdepth_summary;

/* All device and pinned memory is allocated here.  VIL_ERR_DEVICE without a HIP device, VIL_ERR_INVALID_ARGUMENT for a size < 1. */
int vdepth_create(int32_t device, int32_t max_cloud_points, int32_t max_features, vdepth_ctx** out);
void vdepth_destroy(vdepth_ctx* ctx);
/* xyzi: n world-frame points [x y z intensity].  The cloud replaces the resident one and stays until it is replaced; n = 0 gives the
 * "no cloud" state (:109: every depth -1).  VIL_ERR_INVALID_ARGUMENT when n > max_cloud_points; the resident cloud is kept then. */
int vdepth_set_cloud(vdepth_ctx* ctx, int32_t n, const float* xyzi);
/* world_to_lidar, lidar_to_view: row-major float 3 x 4, applied one after the other (step 1).  feat_xyz: n_feat x 3, the undistorted
 * normalised features (z = 1).  depth_out: n_feat floats, -1 where the reference leaves -1.  `out` may be NULL.  One submission on the
 * context's stream: one upload (matrices + features), three kernels, one read-back (counts + depths).
 * VIL_ERR_INVALID_ARGUMENT when n_feat > max_features (nothing is written then). */
int vdepth_register(vdepth_ctx* ctx, const float* world_to_lidar, const float* lidar_to_view, int32_t n_feat, const float* feat_xyz, float* depth_out,
                    vdepth_summary* out);
/* test hook: intermediate results of the last vdepth_register.  sphere_xyzr: the sphere cloud [x y z range] in emission order, `capacity`
 * points of room (VIL_ERR_INVALID_ARGUMENT when that is less than n_sphere); nn3: three sphere indices per feature of the last call in
 * (distance, index) order, -1 -1 -1 for a feature that was not accepted in step 8.  Either pointer may be NULL. */
int vdepth_debug_read(vdepth_ctx* ctx, float* sphere_xyzr, int32_t capacity, int32_t* nn3);
/* measurement hook, as vscan_profile_*: HIP events on the context's stream around the kernels; read returns the launch counts and total
 * durations of {k_depth_project, k_depth_compact, k_depth_query} and resets them */
int vdepth_profile_enable(vdepth_ctx* ctx, int32_t enable);
int vdepth_profile_read(vdepth_ctx* ctx, int64_t* launches3, double* total_ms3);

#ifdef __cplusplus
}
#endif
#endif
