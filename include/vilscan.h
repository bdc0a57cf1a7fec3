/* vilscan.h -- C-ABI of the LOAM feature extraction of mVIL-Fusion's "feature" node: a raw LiDAR scan in, the ring-ordered cloud and the
 * corner / surf feature clouds that vmap_align (vilmap.h) consumes out.
 *
 * Replaces, in lidar_mapping/src/scanRegistration.cpp, PointProcessor::Process (:43-48) = PointToRing + ExtractFeaturePoints, with the
 * helpers of lidar_compensator/src/math_utils.h (:62-91) and PointProcessor.h (:25-41, :77-81):
 *   1 ring sort      PointToRing (:293-416, the non-DEBUG_ORIGIN branch) and the concatenation of :276-290: points with a non-finite x, y or z
 *                    are dropped; ele = atan2f(z, sqrtf(x*x + y*y)); v = (ele * 180 / pi - lower) * ((num_rings - 1) / (upper - lower)) + 0.5
 *                    evaluated in double from the float ele; the point is kept when -1 < v < num_rings and goes to ring int(v) (truncation,
 *                    as ElevationToRing, PointProcessor.h:77-81, which rounds the degrees and the factor to float first: the two agree except
 *                    within ~1e-5 degrees of a ring boundary); points keep their arrival order inside a ring (a stable partition); the rings
 *                    concatenated are the full cloud (cloud_in_rings_).
 *   2 ring mask      rings of <= 2 C + 1 points are skipped (:64; C = num_curvature_regions).  PrepareRing (:510-561), the occlusion /
 *                    parallel-beam mask, with its float-against-double comparisons.  DEVIATION: the reference's
 *                    fill_n(&mask[i + 1], C + 1, 1) writes one element past the ring's end when i = size - C - 1; here the write is clamped
 *                    to the ring.
 *   3 subregions     j = 0..S-1, sp / ep of :78-79, skipped when ep <= sp; PrepareSubregion (:563-621): curvature, the intensity vote (a
 *                    neighbour counts when 1 <= intensity / intensity[i] < 2, which is int(ratio) == 1 for every finite ratio; NaN and
 *                    infinite ratios, undefined in the reference, do not count), the two mask rules of :603-610, ascending sort by
 *                    (curvature, index).  A NaN curvature (coordinates that overflow float) is as undefined here as in the reference.
 *   4 picks          :90-146 with MaskPickedInRing (:623-649): from the high end up to max_corner_less_sharp points with mask == 0 and
 *                    curvature > surf_curv_th / 2 (the first max_corner_sharp are also corner_sharp), then from the low end up to
 *                    max_surf_flat points with mask == 0 and curvature < surf_curv_th / 10; every point of a subregion whose label is <= 0
 *                    is "less flat".
 *   5 output order   ring, subregion, pick order for corner_sharp / corner_less_sharp / surf_flat; ring, subregion, index for less flat:
 *                    the reference's push_back order.
 *   6 downsample     DEVIATION: the reference runs pcl::ApproximateVoxelGrid per ring (:150-167), a hash with eviction whose result depends
 *                    on its table size and on the order of the points.  This library runs an EXACT voxel filter per ring instead: cell =
 *                    floorf(coord * (1.0f / less_flat_filter_size)) per axis (cells beyond the int32 range are out of scope), one output
 *                    point per occupied cell, all four fields averaged (accumulated in double in ring order, divided, rounded once to
 *                    float), cells emitted in the order of their first point.  n_less_flat_raw and the labels describe the cloud BEFORE the
 *                    filter, so steps 1-5 can be checked exactly.
 * All float arithmetic of steps 2-4 is unfused IEEE float32 in the reference's source order: results are bit-reproducible against a
 * scalar float32 restatement (tests/scanreg_ref.py); only atan2f of step 1 is the device library's.
 * A ring holds at most VSCAN_MAX_RING_POINTS points (the ring, its sort keys and the filter's table live in the 160 kB of one compute
 * unit's local memory); a longer ring gives VIL_ERR_UNSUPPORTED, as does the `uneven` ring mapping, which the reference declares
 * (scanRegistration.cpp:19, :697-700) and never implements.
 * Points are float [x y z intensity] (PointXYZI).  Plain C, POD only, host pointers.  Needs a HIP device; there is no CPU fallback. */
#ifndef VILSCAN_H
#define VILSCAN_H
#include <stdint.h>
#include "vilsolve.h"
#ifdef __cplusplus
extern "C" {
#endif

#define VSCAN_MAX_RING_POINTS 4096
#define VSCAN_MAX_RINGS 128
#define VSCAN_NUM_KERNELS 4

typedef struct vscan_ctx vscan_ctx;

typedef struct vscan_config {       /* defaults: PointProcessor.h:34-41 and the 16-ring constructor (scanRegistration.cpp:17) */
    int32_t num_rings;              /* 16 (1..VSCAN_MAX_RINGS) */
    float lower_bound_deg, upper_bound_deg;   /* -15, 15 (main(), :682-689: 32 rings -30.67 / 10.67, 64 rings -24.9 / 2) */
    int32_t num_scan_subregions;    /* 8 (1..256) */
    int32_t num_curvature_regions;  /* 5 (1..32) */
    float surf_curv_th;             /* 1.0 */
    int32_t max_corner_sharp;       /* 3 */
    int32_t max_corner_less_sharp;  /* 30 (0..4096, like the two other quotas) */
    int32_t max_surf_flat;          /* 4 */
    float less_flat_filter_size;    /* 0.2 */
    int32_t uneven;                 /* 0; anything else: VIL_ERR_UNSUPPORTED */
} vscan_config;

typedef struct vscan_cloud {        /* xyzi == NULL: the cloud is not copied out, its count is still returned */
    float* xyzi;                    /* capacity x 4 floats, caller-provided */
    int32_t capacity;               /* in points */
    int32_t count;                  /* out */
} vscan_cloud;

typedef struct vscan_result {
    vscan_cloud cloud;              /* the ring-ordered full cloud */
    int32_t* ring_table;            /* num_rings x [start, count] into `cloud` (NULL: not copied out) */
    int32_t ring_capacity;          /* in rings; needs >= num_rings */
    int32_t num_rings;              /* out */
    int8_t* labels;                 /* one PointLabel per point of `cloud`: 2 sharp, 1 less sharp, 0 less flat / none, -1 flat (NULL: not copied) */
    int32_t label_capacity;         /* in points; needs >= cloud.count */
    int32_t n_less_flat_raw;        /* out: less-flat points before the voxel filter */
    vscan_cloud corner_sharp, corner_less_sharp, surf_flat, surf_less_flat;
} vscan_result;

void vscan_default_config(vscan_config* cfg);
/* max_points: the largest scan vscan_extract will be given (all device and pinned memory is allocated here).
 * VIL_ERR_DEVICE without a HIP device, VIL_ERR_INVALID_ARGUMENT for a config outside the ranges above. */
int vscan_create(int32_t device, const vscan_config* cfg, int32_t max_points, vscan_ctx** out);
void vscan_destroy(vscan_ctx* ctx);
/* xyzi: n raw points in arrival order.  One submission on the context's stream (upload, four kernels, one read-back).  Every count of
 * `out` is set whenever the device work succeeded; VIL_ERR_INVALID_ARGUMENT (VIL_ERR_INVALID for short) when n > max_points or a
 * capacity is smaller than its count (no array is written then), VIL_ERR_UNSUPPORTED when a ring exceeds VSCAN_MAX_RING_POINTS. */
int vscan_extract(vscan_ctx* ctx, int32_t n, const float* xyzi, vscan_result* out);
/* measurement hook, as vmap_profile_*: HIP events on the library's stream around the kernels; read returns the launch counts and total
 * durations of {k_scan_ring_id, k_scan_ring_sort, k_scan_features, k_scan_gather} and resets them */
int vscan_profile_enable(vscan_ctx* ctx, int32_t enable);
int vscan_profile_read(vscan_ctx* ctx, int64_t* launches4, double* total_ms4);

#ifdef __cplusplus
}
#endif
#endif
