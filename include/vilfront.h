/* vilfront.h -- C-ABI of the scan-to-scan LiDAR front end as one resident call: from a raw scan to the alignment, the fitness score and
 * the numbers the ICP constraint is built from.
 *
 * Replaces, in vils_estimator's Estimator::processLidar (estimator.cpp:122-436), everything between the keyframe lookup and the
 * constraint: TransformToEnd + pcl::removeNaNFromPointCloud (:233-237, lidar_frontend.cpp:1001-1041), pcl::ApproximateVoxelGrid
 * (:243-246), the two-frame all_lidar_frame (:250-266), FastVGICP::align (:269-300) and getFitnessScore() (:303).  It is a composition:
 *   de-skew + ordered compaction   new here (k_front_deskew, k_front_scan, k_front_scatter)
 *   filter A(leaf, hist_size)      vilcloud.h, device to device
 *   previous source -> target      vgicp_promote_source (vilvgicp_voxel.h) and the fitness cloud's promotion (villoop.h)
 *   covariances (k = 20), align    vilvgicp.h
 *   fitness                        vloop_score (villoop.h)
 * The host arithmetic around the call (the de-skew motion, the predicted guess, the constraint deque) is include/vilfront_shim.hpp; the
 * constraint's mode and factor are include/vilicp_shim.hpp.  STAYS ON THE HOST: FindNearest2ID and the all_image_frame lookups
 * (:135-164), the LiDAR-IMU extrinsic initialisation (:438 onwards).  Account of the stages and the measurements: docs/lidarfront.md.
 *
 * ARITHMETIC CONTRACT OF THE DE-SKEW.  Unfused IEEE float32 in the order written; p = [x y z intensity]; the motion is the float
 * quaternion e = (w, x, y, z) and the float translation t that TransformToEnd receives; time_factor = (float)(1.0 / lidar_time_step),
 * the division in double (estimator.cpp:190); min_distance and max_distance are doubles.
 *   0 DEVIATION: a point whose intensity is NaN or not in [-2^31, 2^31) is rejected (the reference casts it to int, which is undefined).
 *   1 distance = sqrtf(x * x + y * y).  lidar_frontend.cpp is compiled under `using namespace std` (initial_alignment.h:16) and the
 *     argument is a float, so the call resolves to std::sqrt(float); the float result is widened and compared with min and max in double.
 *   2 s = time_factor * (intensity - (float)(int)intensity).  The conversion truncates towards zero: a negative intensity with a
 *     fractional part gives s < 0 (with a positive time_factor).
 *   3 the point is REJECTED when s < 0.0f || (double)s > 1.001 || (double)distance < min || (double)distance > max.  s is a float and
 *     1.001 a double literal: the float is widened, the literal is not rounded.  A NaN coordinate fails none of the four comparisons:
 *     it passes this gate and is removed by step 9.
 *   4 x = x - s * t.x, and y, z likewise.
 *   5 q_s = identity.slerp(s, e), Eigen's QuaternionBase::slerp: d = e.w (the dot product with the identity); absD = fabsf(d);
 *     if absD >= 1.0f - FLT_EPSILON: scale0 = 1.0f - s, scale1 = s; otherwise theta = acosf(absD), sinTheta = sinf(theta),
 *     scale0 = sinf((1.0f - s) * theta) / sinTheta, scale1 = sinf(s * theta) / sinTheta.  If d < 0.0f: scale1 = -scale1.
 *     q_s = (w: scale0 + scale1 * e.w, x: scale1 * e.x, y: scale1 * e.y, z: scale1 * e.z).
 *   6 c = conjugate(q_s) = (q_s.w, -q_s.x, -q_s.y, -q_s.z), then normalised: n2 = ((c.x * c.x + c.y * c.y) + c.z * c.z) + c.w * c.w,
 *     every component divided by sqrtf(n2) when n2 > 0.0f (Eigen's normalized()).
 *   7 the point is rotated by c, then by e (NOT normalised), each as Eigen's quaternion * vector: with u = q.vec and v the point,
 *     a = cross(u, v); a = a + a; b = cross(u, a); result = (v + q.w * a) + b, componentwise, cross(u, v) = (u.y * v.z - u.z * v.y,
 *     u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x).
 *   8 x = x + t.x, and y, z likewise; intensity = (float)(int)intensity.
 *   9 removeNaNFromPointCloud: the point is REMOVED when any of x, y, z is not finite after step 8.  The survivors keep their input order.
 * The slerp, the normalisation and the rotation are restatements of Eigen 3.3's text; they are checked against a 50-digit evaluation
 * of THIS text (tests/lidarfront_ref.py), not against Eigen's bits (Eigen sums the four squares of step 6 in its packet order).
 * acosf and sinf are the device's: steps 4-8 are held to a tolerance (16 x the error of the float32 NumPy restatement), the kept mask,
 * the order, the intensities and everything after the de-skew to raw bytes.
 *
 * HOST WAITS per accepted vfront_push_scan with a previous scan: seven, eight when the fitness target is large enough for a search
 * grid.  (1) the counts after the filter; (2) the voxel count of the promoted target; (3) the fitness target's copy (and its grid: one
 * more); (4) the covariances of the new source; (5) the fitness source's copy; (6) the alignment's record; (7) the score's record.  The
 * first accepted scan takes (1), (4), (5).  Up: 16 B per raw point; the motion and the options travel as kernel arguments.  Down: the
 * 64-byte header, the alignment's record and the score's.  The streams of the four contexts are ordered by events around the filter
 * and by these waits everywhere else (csrc/vilcloud_stage.hpp, vilvgicp_stage.hpp, villoop_stage.hpp say which).
 *
 * Plain C, POD only, host pointers.  Status codes are those of vilsolve.h.  Needs a HIP device; there is no CPU fallback. */
#ifndef VILFRONT_H
#define VILFRONT_H
#include <stdint.h>
#include "vilcloud.h"
#include "villoop.h"
#include "vilsolve.h"
#include "vilvgicp.h"
#ifdef __cplusplus
extern "C" {
#endif

#define VFRONT_NUM_KERNELS 4
#define VFRONT_KNN 20              /* neighbours of a source covariance (fast_gicp's k_correspondences_) */
/* stages of vfront_debug_read */
#define VFRONT_DBG_DESKEWED 0      /* steps 0-9 (the raw scan with deskew = 0) */
#define VFRONT_DBG_FILTERED 1      /* filter A on it: what becomes the alignment's source */

typedef struct vfront_ctx vfront_ctx;

typedef struct vfront_motion {
    float q[4];                    /* transform_es_q as (w, x, y, z) */
    float t[3];                    /* transform_es_t */
    float reserved;
} vfront_motion;

typedef struct vfront_options {
    int32_t deskew;                /* 1; 0 is the lidar_init_flag == true branch: the raw scan goes to the filter unchanged */
    int32_t hist_size;             /* 512 */
    double lidar_time_step;        /* 0.1  LidarTimeStep */
    double min_distance;           /* 0.5  MinDistance */
    double max_distance;           /* 70.0 MaxDistance */
    double resolution;             /* 0.5  setResolution, estimator.cpp:270 */
    float leaf;                    /* 0.3f LeafSize */
    int32_t reserved;
    vgicp_options reg;             /* vgicp_default_options */
} vfront_options;

typedef struct vfront_summary {
    int32_t n_raw;                 /* points handed over */
    int32_t n_kept;                /* after the de-skew (n_raw with deskew = 0) */
    int32_t n_filtered;            /* after filter A */
    int32_t accepted;              /* 0: the filtered cloud is empty, the resident pair is unchanged */
    int32_t aligned;               /* 0: there was no previous scan; T is the identity, fitness 0, n_used 0, reg zeroed */
    int32_t n_used;                /* points behind the fitness */
    double fitness;                /* getFitnessScore() at T, max_range = DBL_MAX; read whether or not the alignment converged */
    double T[16];                  /* getFinalTransformation(): the alignment's result rounded to float, row-major, source -> target */
    vgicp_summary reg;
} vfront_summary;

/* All device and pinned memory for scans of up to max_scan_points points is allocated here, with a private vcloud_ctx, vgicp_ctx and
 * vloop_ctx.  VIL_ERR_INVALID_ARGUMENT for max_scan_points < 1 or more than 2^27 or out = NULL (checked first), VIL_ERR_DEVICE without a
 * HIP device. */
int vfront_create(int32_t device, int32_t max_scan_points, vfront_ctx** out);
void vfront_destroy(vfront_ctx* ctx);
/* no resident scan: the next accepted scan is a first one.  Also what recovers a context after a VIL_ERR_DEVICE (below). */
int vfront_reset(vfront_ctx* ctx);
void vfront_default_options(vfront_options* opts);
/* The fitness search's grid threshold (vloop_set_grid of the private context): targets of at least min_points filtered points are
 * searched through a uniform grid of edge `cell`.  Default 1024, 0.5. */
int vfront_set_grid(vfront_ctx* ctx, int32_t min_points, double cell);
/* One scan whose bracketing keyframes the caller found.  xyzi: n x 4 floats.  guess: row-major 4 x 4 double, rounded to float before
 * use; NULL (the align(*aligned) branch, :299) is the identity.  opts may be NULL (the defaults), `summary` may be NULL.
 *   1 de-skew (when opts.deskew), 2 filter A(leaf, hist_size), 3 the previous scan's sources become the targets, 4 the filtered cloud
 *   becomes the sources (covariances from its VFRONT_KNN nearest neighbours), 5 vgicp_align from the guess and vloop_score at its
 *   float-rounded result when there is a target, 6 this scan is the previous scan.
 * Every argument is checked before any device work: VIL_ERR_INVALID_ARGUMENT for n < 0, n > max_scan_points, a NULL it needs, a motion,
 * guess or option that is not finite, a lidar_time_step, leaf or resolution that is not positive, a hist_size vcloud_filter refuses or a
 * neighbor_mode vgicp_align refuses.  A refused call leaves all resident state, the debug stages included, alone.
 * A scan whose filtered cloud is empty returns VIL_OK with accepted = 0; a filtered cloud with a non-finite centroid (an overflow of
 * filter A's sums) returns VIL_ERR_NON_FINITE; both leave the resident pair alone and the debug stages hold the refused scan.
 * A status of vgicp_align or vloop_score other than VIL_ERR_DEVICE (VIL_ERR_NON_FINITE from a degenerate pair) is returned with the scan
 * stored as the previous scan, aligned = 0.
 * VIL_ERR_DEVICE from step 3 onwards leaves the pair half exchanged: the context then answers every vfront_push_scan with
 * VIL_ERR_DEVICE until vfront_reset, after which the next accepted scan is a first one. */
int vfront_push_scan(vfront_ctx* ctx, int32_t n, const float* xyzi, const vfront_motion* motion, const double* guess, const vfront_options* opts,
                     vfront_summary* summary);
/* The de-skewed cloud with its removed points gone, which the reference writes back into the caller's cloud (:234-237): n_kept x 4
 * floats of the last scan that reached the device.  VIL_ERR_INVALID_ARGUMENT when capacity (in points) is below *n, which is still set. */
int vfront_read_deskewed(vfront_ctx* ctx, float* out_xyzi, int32_t capacity, int32_t* n);
/* test hook: one of the VFRONT_DBG_* stages of that scan, float [x y z intensity] */
int vfront_debug_read(vfront_ctx* ctx, int32_t stage, float* out_xyzi, int32_t capacity, int32_t* n);
/* measurement hook, as vcloud_profile_*: HIP events on the context's stream around the launches; read returns the launch counts and
 * total durations of {k_front_deskew, k_front_scan, k_front_scatter, k_front_xyz} and resets them */
int vfront_profile_enable(vfront_ctx* ctx, int32_t enable);
int vfront_profile_read(vfront_ctx* ctx, int64_t* launches4, double* total_ms4);

#ifdef __cplusplus
}
#endif
#endif
