/* villmap.h -- C-ABI of lidar_mapping's local cube map, resident on the device: process() of lidar_mapping/src/localMapping.cpp from
 * transformAssociateToMap() (:338) to the publication decision (:893-982) as one call per scan.
 *
 * The 11 x 11 x 7 array of cubes, their points and the registration map stay on the device between scans.  Per scan the two feature
 * clouds (/laser_cloud_less_sharp and /laser_cloud_less_flat: corner_less_sharp and surf_less_flat of vscan_result) and the odometry
 * pose go up, a summary with the mapped pose comes back; the map's points cross the bus only when vlmap_read_published asks for a
 * published local map.
 *
 * OUT OF SCOPE (stays with the caller): the ROS queues and their time matching (:263-334); laserCloudFullRes and its two topics; the
 * path / tf / Midend.txt output; the commented-out outlier filter; handing the published map to vgmap_* device to device (it is read
 * back and handed to vgmap_add_scan by the caller).
 *
 * A RESTATEMENT WITH A WRITTEN CONTRACT, checked bit for bit against a sequential restatement of THIS text (tests/localmap_ref.py) and
 * against the chain of public calls (vcloud_filter, vmap_set_map, vmap_align), not against PCL's bits.
 *
 * ARITHMETIC CONTRACT.  Unfused IEEE arithmetic in the order written.  Points are float [x y z intensity].  A cube is addressed as
 * (i, j, k), 0 <= i < VLMAP_W, 0 <= j < VLMAP_H, 0 <= k < VLMAP_D, index = i + VLMAP_W * j + VLMAP_W * VLMAP_H * k.  Class 0 is corner,
 * class 1 is surf.  The state between scans: the cubes, the cube of the world's origin (cenW, cenH, cenD: laserCloudCenWidth / Height /
 * Depth, 5 / 5 / 3 at the start), q_wmap_wodom / t_wmap_wodom, frameCount, first_odom, the last published pose and its frame count.
 *
 *  1 GUESS (:158-162), on the host in double: q_w_curr = q_wmap_wodom * q_wodom (Hamilton product in Eigen's order of operations),
 *    t_w_curr = q_wmap_wodom * t_wodom + t_wmap_wodom (Eigen's quaternion * vector: uv = 2 (q.vec x v); v + w uv + q.vec x uv).
 *  2 CENTRE AND SHIFT (:341-536).  cI = int((t.x + H) / cube_length) + cenW, and `if (t.x + H < 0) cI--`; cJ likewise with cenH, cK
 *    with cube_height and cenD.  The division is in double, int() truncates.
 *    QUIRK (reproduced): the reference writes `HalfCubeLength = 1 / 2 * CubeLength`, an integer division, so H = 0.0.  Cube boundaries
 *    lie on multiples of the cube length, not half a cube off; a coordinate that is exactly a negative multiple lands one cube lower
 *    than its neighbours to the right (int(-1.0) - 1); -0.0 lands in cube 0 (-0.0 < 0 is false).
 *    Then the six while loops: while cI < 3, every cube takes the contents of its lower neighbour along that axis, slot 0 is
 *    emptied, cI and cenW go up by one; while cI >= size - 3, the other way round and the last slot is emptied.  A jump of several
 *    cubes runs a loop several times.  Both classes shift together.  Order: I up, I down, J up, J down, K up, K down.
 *    The host decides the shifts (it knows t_w_curr) and applies them to its table of the cubes' places; no point moves.
 *  3 FROM-MAP (:538-568).  The valid cubes are i = cI-2 .. cI+2 (outer loop), j = cJ-2 .. cJ+2, k = cK-1 .. cK+1 (inner loop), those
 *    inside the array.  Their clouds, concatenated in that order, each cube's points in stored order, become the map of the private
 *    vmap_ctx, device to device, followed by the same grid_build_adaptive as vmap_set_map.
 *  4 STACK (:570-582).  Filter A(line_res, hist_size) of vilcloud.h on the corner cloud, A(plane_res, hist_size) on the surf cloud.
 *  5 ALIGN (:586-793).  Only when n_corner_from_map > 10 && n_surf_from_map > 50: exactly what vmap_align runs on that map and those
 *    stacks from the guess (both rounds, same kernels, same grids; vilmap.h says how its update differs from the reference's).
 *    Otherwise the pose stays the guess.  Then transformUpdate() (:164-168) on the host in double: q_wmap_wodom = q_w_curr *
 *    q_wodom^-1 (the conjugate divided by the squared norm, as Eigen's inverse()), t_wmap_wodom = t_w_curr - q_wmap_wodom * t_wodom.
 *  6 ADD (:802-848).  Each stack point p goes through pointAssociateToMap: x, y, z promoted to double; per row r of the 3 x 4 matrix
 *    [R | t], ((r0 x + r1 y) + r2 z) + r3 in double; rounded to float; the intensity unchanged.  The matrix is the rotation matrix and
 *    translation the last solve left on the device; when no one-launch solve ran, the host's quat_to_R of (q_w_curr, t_w_curr).
 *    VLMAP_DBG_MATRIX reads the one that was used.  The cube of the FLOAT point is found as in step 2 with cenW, cenH, cenD as the
 *    shifts left them: double division, truncation, decrement when negative.  Points outside the array are dropped.
 *    DEVIATION: a point with a coordinate that is not finite after the transform is dropped too (the reference casts it to int).
 *    Accepted points are appended to their cube in stack order.  They also land in cubes that are not valid this scan.
 *  7 REFILTER (:853-868).  Every valid cube (step 3's list) is replaced by A(line_res, hist_size) (corner) or A(plane_res, hist_size)
 *    (surf) of itself, the appended points last: each cube a filter A of its own, byte-equal to vcloud_filter of that cube alone.  A cube
 *    that is not valid keeps its appended points unfiltered for as long as it stays invalid.
 *  8 PUBLICATION (:893-982, FOR_GLOBAL defined).  While first_odom: the last pose is the current one, and when frameCount >=
 *    publish_first_frame the map is published and first_odom cleared.  Afterwards: d = R^T (t_last - t_w_curr) with R the host's
 *    quat_to_R of q_w_curr; publish when sqrt((dx dx + dy dy) + dz dz) > publish_distance || frameCount - last_frame_count >
 *    publish_frames.  Publishing: all cubes in index order, corner then surf per cube, form the map; every cube is emptied; the
 *    sensor-frame copy (/local_map, :949-959) is per row c of R^T: ((R0c dx + R1c dy) + R2c dz) with d = (double)p - t_w_curr, rounded to
 *    float, the intensity unchanged; the last pose becomes the current one, last_frame_count = frameCount; q_wmap_wodom, t_wmap_wodom
 *    become identity / zero.
 *  9 frameCount++.
 *
 * A REFUSED CALL CHANGES NOTHING: the cubes, the state and the last published map are as before when vlmap_push_scan returns anything
 * but VIL_OK (the debug stages may be overwritten).  Plain C, POD only, host pointers.  Status codes are those of vilsolve.h.  Needs a
 * HIP device; there is no CPU fallback. */
#ifndef VILLMAP_H
#define VILLMAP_H
#include <stdint.h>
#include "vilmap.h"
#include "vilsolve.h"
#ifdef __cplusplus
extern "C" {
#endif

#define VLMAP_W 11               /* laserCloudCenWidth = 5 */
#define VLMAP_H 11               /* laserCloudCenHeight = 5 */
#define VLMAP_D 7                /* laserCloudCenDepth = 3 */
#define VLMAP_CUBES (VLMAP_W * VLMAP_H * VLMAP_D)
#define VLMAP_MAX_VALID 75       /* 5 x 5 x 3 */
#define VLMAP_NUM_KERNELS 6
/* stages of vlmap_debug_read */
#define VLMAP_DBG_CORNER_STACK 0 /* step 4 */
#define VLMAP_DBG_SURF_STACK 1
#define VLMAP_DBG_CORNER_FROM_MAP 2 /* step 3 */
#define VLMAP_DBG_SURF_FROM_MAP 3
#define VLMAP_DBG_MATRIX 4       /* step 6: 12 doubles, row-major 3 x 4 [R | t], read as 6 "points" of 4 floats' bytes: see vlmap_debug_read */
/* frames of vlmap_read_published */
#define VLMAP_FRAME_WORLD 0      /* /laser_cloud_map */
#define VLMAP_FRAME_SENSOR 1     /* /local_map */

typedef struct vlmap_ctx vlmap_ctx;

typedef struct vlmap_config {
    float line_res;              /* 0.2f (:1099) */
    float plane_res;             /* 0.4f (:1100) */
    int32_t hist_size;           /* 512: pcl's histsize_ */
    int32_t publish_first_frame; /* 10 (:900) */
    double cube_length;          /* 10.0 (I and J) */
    double cube_height;          /* 5.0 (K) */
    double publish_distance;     /* 2.0 (:912) */
    int32_t publish_frames;      /* 30 (:912) */
    int32_t max_scan_points;     /* per class, default 1 << 15 */
    int32_t max_map_points;      /* per class, all cubes together, default 1 << 19 */
    int32_t reserved;
} vlmap_config;

typedef struct vlmap_summary {
    double q_w_curr[4];          /* x y z w */
    double t_w_curr[3];
    int32_t shift[3];            /* cubes the array's contents moved along I, J, K: +1 per pass of a "centre < 3" loop, -1 per pass of the other */
    int32_t n_corner_from_map, n_surf_from_map;
    int32_t n_corner_stack, n_surf_stack;
    int32_t aligned;             /* 0 when :586 fails */
    int32_t n_corner_added, n_surf_added;     /* stack points that fell inside the array */
    int32_t n_corner_map, n_surf_map;         /* all cubes, after step 7 (before step 8 empties them) */
    int32_t published;
    int32_t frame_count;         /* after step 9 */
    int32_t reserved;
    vmap_summary align;          /* zero when aligned is 0 */
} vlmap_summary;

void vlmap_default_config(vlmap_config* cfg);
/* All device and pinned memory is allocated here.  cfg may be NULL (the defaults).  VIL_ERR_DEVICE without a HIP device;
 * VIL_ERR_INVALID_ARGUMENT for a resolution vcloud_filter would refuse, a cube size or a publish distance that is not finite and
 * positive (the distance may be 0), max_scan_points < 1, max_map_points < max_scan_points or more than 2^24 points. */
int vlmap_create(int32_t device, const vlmap_config* cfg, vlmap_ctx** out);
void vlmap_destroy(vlmap_ctx* ctx);
/* empty cubes, centre 5 / 5 / 3, q_wmap_wodom identity, frameCount 0, first_odom true, nothing published */
int vlmap_reset(vlmap_ctx* ctx);
/* Steps 1-9.  `solver` is vmap_align's.  opts may be NULL: vil_default_options with max_iterations = 4 (:772).  summary may be NULL.
 * VIL_ERR_INVALID_ARGUMENT for n > max_scan_points, a non-finite pose, a zero quaternion, or a guessed position (step 1) more than
 * 65536 cubes from the array's centre along an axis (no map reaches there, and step 2's loops would run once per cube);
 * VIL_ERR_CAPACITY when the points in all cubes of a class (the previous summary's n_*_map) plus that class's n could exceed
 * max_map_points, decided before any device work. */
int vlmap_push_scan(vlmap_ctx* ctx, vil_ctx* solver, int32_t n_corner, const float* corner_xyzi, int32_t n_surf, const float* surf_xyzi,
                    const double* q_wodom_xyzw, const double* t_wodom, const vil_options* opts, vlmap_summary* summary);
/* The last published map in one of the VLMAP_FRAME_* (nothing before the first publication and after vlmap_reset).
 * VIL_ERR_INVALID_ARGUMENT when capacity (in points) is below *n, which is still set then. */
int vlmap_read_published(vlmap_ctx* ctx, int32_t frame, float* out_xyzi, int32_t capacity, int32_t* n);
/* test hooks: one cube (cls 0 corner, 1 surf; index as above), and one of the VLMAP_DBG_* stages of the last push.  VLMAP_DBG_MATRIX
 * is 12 doubles: *n = 6 and out_xyzi receives 96 bytes. */
int vlmap_read_cube(vlmap_ctx* ctx, int32_t cls, int32_t index, float* out_xyzi, int32_t capacity, int32_t* n);
int vlmap_debug_read(vlmap_ctx* ctx, int32_t stage, float* out_xyzi, int32_t capacity, int32_t* n);
/* TEST HOOK ONLY, not part of the mapping interface: it rewrites the map's state directly.  Replaces the contents of one cube by n raw
 * points, unfiltered, as if they had been appended while the cube was not valid (the stacks are filtered before they reach a cube, so
 * no sequence of pushes can build such a cube).  The points go behind every cube the class's pool holds and the replaced cube's old
 * place becomes a hole: the pool stays unpacked until the next push lays it out again, so repeated writes without a push run into
 * VIL_ERR_CAPACITY although the cubes together would fit. */
int vlmap_debug_write_cube(vlmap_ctx* ctx, int32_t cls, int32_t index, int32_t n, const float* xyzi);
/* measurement hook, as vcloud_profile_*: launch counts and total durations of {k_lmap_gather, k_lmap_place, k_lmap_layout,
 * k_lmap_append, k_lmap_refilter, k_lmap_publish}; read resets them.  The stacks' filter and the alignment are the cloud and map rows'
 * kernels and are not in this list. */
int vlmap_profile_enable(vlmap_ctx* ctx, int32_t enable);
int vlmap_profile_read(vlmap_ctx* ctx, int64_t* launches6, double* total_ms6);

#ifdef __cplusplus
}
#endif
#endif
