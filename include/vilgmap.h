/* vilgmap.h -- C-ABI of the global map of lidar_mapping, resident on the device: the structure the global-mapping node inserts every scan
 * into, cuts its registration reference from and regenerates from the keyed scans after a loop closure.
 *
 * Where the reference does these things (lidar_mapping/src/globalMappingOcTree.cpp = O, globalMappingIkdTree.cpp = I):
 *   O:287, I:281           keyed_scans.insert(key, scan in the sensor frame)                                  -> vgmap_add_scan
 *   O:694-704, I:668-672   InsertPoints: the scan, moved into the world by transformPointsCloud2Frame; O keeps a point only when its
 *                          0.05 m voxel (util.h:79) is still empty, I keeps every point                      -> vgmap_insert, vgmap_insert_key
 *   O:706-757              ApproxNearestNeighbors: 0.5 m radius search (util.h:80) per query point, the union thinned to one point per
 *                          0.3 m voxel (util.h:81)                                                            -> vgmap_reference, VGMAP_REF_RADIUS
 *   I:673-707              the 5 nearest map points per query point with max_dist 1.5                         -> vgmap_reference, VGMAP_REF_KNN
 *   O:249, I:246           the reference moved into the sensor frame by current_localization.inv()            -> vgmap_reference's T_out
 *   O:296-331, O:416, I:289-310, I:396   after a loop closure or a z drift above 1 m (I: 0.5 m): GetMaximumLikelihoodPoints, reset, and
 *                          InsertPoints / Build of every keyed scan at its optimised pose                     -> vgmap_rebuild
 * The poses vgmap_rebuild takes are what vpgo_get_poses (vilpgo.h) returns, as matrices (Pose6D <-> matrix: vilpgo_shim.hpp).
 *
 * ARITHMETIC CONTRACT.  tests/globalmap_ref.py restates it in NumPy; the library's results equal it bit for bit.
 *   1 Transform.  T is a row-major 4x4 double (only its first three rows are read).  A float point (x, y, z) is promoted to double,
 *     q_r = ((m_r0 * x + m_r1 * y) + m_r2 * z) + m_r3 for r = 0, 1, 2, unfused, and q_r is rounded to float.
 *     DEVIATION: PCL is not part of the reference tree; pcl::transformPointCloud with a Matrix4d is restated, not transcribed.
 *   2 Voxel of a float point p at resolution res: c_a = (int64)floor(((double)p_a - origin_a) / (double)res) per axis, IEEE double
 *     division.  |c_a| < 2^20 is required (VGMAP_VOXEL_LIMIT).  The voxel's key is ((c_x + 2^20) << 42) | ((c_y + 2^20) << 21) | (c_z + 2^20).
 *     DEVIATION: PCL's octree anchors its grid where its bounding box was first placed (as far as can be recalled the first point minus
 *     half a voxel; its source is not at hand and this is unverified).  Here the anchor is the `origin` option.
 *   3 Insert.  The map holds n_map points.  Input point i (after step 1) survives iff no map point lies in its voxel and no input point
 *     j < i lies in its voxel; the survivors are appended in ascending i.  This is the sequential loop of O:694-704.  On the device: one
 *     integer atomicMin of the global index n_map + i into the voxel's slot of an open-addressing table, then an ordered compaction; no
 *     floating-point atomics; the result depends neither on the scheduling nor on the slot layout.  map_resolution <= 0: every point
 *     survives (the IkdTree variant).
 *   4 Rebuild.  Map and table are emptied; the stored scans of `keys`, each transformed by its T, are concatenated in the given order and
 *     inserted as ONE input of step 3 (one pass over all keyed points).  Bit-identical to vgmap_clear followed by vgmap_insert_key per key
 *     in that order.
 *   5 Reference, VGMAP_REF_RADIUS.  The query points are transformed by step 1; d2 is the unfused float (dx * dx + dy * dy) + dz * dz.
 *     U = the map points j with d2 <= (float)(radius * radius) for at least one query point.  Of the points of U that share a voxel
 *     (step 2 at ref_resolution) the smallest j is kept; the output is in ascending j.  ref_resolution <= 0: all of U.
 *     DEVIATION: the reference keeps whichever point of a voxel its octree traversal meets first; not reproducible without PCL.
 *   6 Reference, VGMAP_REF_KNN.  For each query point in input order: its k smallest (d2, j) in lexicographic order among the map points
 *     with d2 <= (float)max_dist.  QUIRK reproduced: ikd_Tree.cpp:1087 compares the SQUARED distance with the unsquared max_dist (its box
 *     pruning at max_dist^2, :1067, is wider and changes nothing).  A map point found from two query points appears twice (I:693).
 *     DEVIATION: ties go to the smaller j, where the tree breaks them by traversal.
 *   7 Hand-over.  When T_out is given every output point is transformed by step 1 with T_out; ref_idx are map indices.
 *
 * ERRORS are decided before the map changes: a refused call leaves map, table and stored scans as they were.
 *   VIL_ERR_INVALID_ARGUMENT  a size outside 1 .. max_*, an unknown or duplicate key, keys that do not ascend strictly, NaN options, an
 *                             unknown mode, k outside 1 .. VGMAP_MAX_K, a radius outside (0, 1024]; a voxel index outside 2^20 (this
 *                             one is found on the device: the first kernel of the submission raises a flag, every later kernel
 *                             returns at once on it)
 *   VIL_ERR_NON_FINITE        a non-finite coordinate or entry of T / T_out
 *   VIL_ERR_CAPACITY          n_map + n > max_map_points, n being the input's size BEFORE thinning.  Conservative on purpose: with it the
 *                             table (at least 2 * max_map_points slots) can never fill and no roll-back is needed.  Also: the keyed
 *                             points of a rebuild exceed max_map_points; a scan store that is full (max_keys, max_keyed_points);
 *                             n_ref > max_ref_points (n_ref is set, nothing is copied).
 * OUT OF SCOPE, left with the caller: pcl::ApproximateVoxelGrid (O:237-240, O:715-718: a hash with eviction whose result depends on
 * its table size; the caller passes filtered clouds), the floor bookkeeping (key_floor), publishing and serialisation.
 * The table: power-of-two slot count >= 2 * max_map_points, home slot = the upper half of key * 0x9E3779B97F4A7C15 masked to the
 * table, linear probing with wrap-around, every probe loop bounded by the slot count.
 * Plain C, POD only, host pointers.  Needs a HIP device; there is no CPU fallback. */
#ifndef VILGMAP_H
#define VILGMAP_H
#include <stdint.h>
#include "vilsolve.h"
#ifdef __cplusplus
extern "C" {
#endif

#define VGMAP_NUM_KERNELS 13
#define VGMAP_MAX_K 64             /* step 6 */
#define VGMAP_VOXEL_LIMIT (1 << 20)
#define VGMAP_REF_RADIUS 0
#define VGMAP_REF_KNN 1

typedef struct vgmap_ctx vgmap_ctx;

typedef struct vgmap_config {
    int32_t max_map_points;
    int32_t max_scan_points;       /* per vgmap_add_scan / vgmap_insert / vgmap_reference call */
    int32_t max_keys;
    int32_t max_keyed_points;      /* sum over the stored scans */
    int32_t max_ref_points;
    float map_resolution;          /* 0.05, util.h:79; <= 0: no thinning (the IkdTree variant) */
    double origin[3];              /* step 2's anchor, for map_resolution and ref_resolution alike */
} vgmap_config;

typedef struct vgmap_ref_options {
    int32_t mode;                  /* VGMAP_REF_RADIUS | VGMAP_REF_KNN */
    int32_t k;                     /* 5, I:686 */
    double radius;                 /* 0.5, util.h:80 */
    float ref_resolution;          /* 0.3, util.h:81; <= 0: no thinning */
    float max_dist;                /* 1.5, compared with the squared distance (step 6) */
} vgmap_ref_options;

/* All device and pinned memory is allocated here; only the search grid's work space grows on demand.  VIL_ERR_INVALID_ARGUMENT for a
 * NULL pointer, a size <= 0, max_map_points > 2^29, max_scan_points > 2^24 or a NaN / infinite resolution or origin (checked first), VIL_ERR_DEVICE without a HIP device. */
int vgmap_create(int32_t device, const vgmap_config* config, vgmap_ctx** out);
void vgmap_destroy(vgmap_ctx* ctx);
/* 1 << 22 map points, 1 << 17 scan points, 4096 keys, 1 << 24 keyed points, 1 << 18 reference points, 0.05, origin 0 */
void vgmap_default_config(vgmap_config* config);
void vgmap_default_ref_options(vgmap_ref_options* o);      /* VGMAP_REF_RADIUS, 5, 0.5, 0.3, 1.5 */
/* store a scan (sensor frame, n x 3 floats) under `key` on the device */
int vgmap_add_scan(vgmap_ctx* ctx, int32_t key, int32_t n, const float* xyz);
/* steps 1 and 3 of n host points; one submission, one read-back of the new n_map */
int vgmap_insert(vgmap_ctx* ctx, int32_t n, const float* xyz, const double* T16);
/* the same for a stored scan, without an upload */
int vgmap_insert_key(vgmap_ctx* ctx, int32_t key, const double* T16);
/* steps 5 - 7 for n query points (sensor frame) at pose T16.  T_out16 may be NULL.  n_ref: the number of output points; ref_xyz:
 * room for max_ref_points x 3 floats; ref_idx: room for max_ref_points, may be NULL.  An empty map gives n_ref = 0. */
int vgmap_reference(vgmap_ctx* ctx, int32_t n, const float* xyz, const double* T16, const vgmap_ref_options* options, const double* T_out16, int32_t* n_ref, float* ref_xyz,
                    int32_t* ref_idx);
/* step 4.  keys: n_keys >= 1 stored keys, strictly ascending; T16s: n_keys x 16 doubles */
int vgmap_rebuild(vgmap_ctx* ctx, int32_t n_keys, const int32_t* keys, const double* T16s);
int vgmap_size(vgmap_ctx* ctx, int32_t* n_map, int32_t* n_keys, int32_t* n_keyed_points);      /* each may be NULL */
int vgmap_get_points(vgmap_ctx* ctx, int32_t first, int32_t n, float* xyz);                     /* map points first .. first + n - 1 */
int vgmap_clear(vgmap_ctx* ctx);                                                                /* empties map and table; the stored scans stay */
/* measurement hook, as vloop_profile_*: read returns launch counts and total durations of {k_gmap_xform, k_gmap_claim, k_gmap_survive,
 * k_gmap_scan, k_gmap_append, k_gmap_wipe, grid (the three kernels of the search grid's rebuild), k_gmap_radius, k_gmap_thin,
 * k_gmap_pick, k_gmap_emit, k_gmap_unclaim, k_gmap_knn} and resets them */
int vgmap_profile_enable(vgmap_ctx* ctx, int32_t enable);
int vgmap_profile_read(vgmap_ctx* ctx, int64_t* launches13, double* total_ms13);

#ifdef __cplusplus
}
#endif
#endif
