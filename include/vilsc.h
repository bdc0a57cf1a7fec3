/* vilsc.h -- C-ABI of the Scan Context place recognition of mVIL-Fusion's lidar_mapping: one down-sampled keyframe scan in, one
 * 20 x 60 descriptor appended to a device-resident database; the newest entry is then searched for against the older ones and a small
 * result record comes back (loop id, column shift = yaw, distance).
 *
 * Replaces SCManager (lidar_mapping/include/scancontext/Scancontext.{h,cpp}) at its two call sites in globalMappingIkdTree.cpp:
 *   :287  scManager.makeAndSaveScancontextAndKeys(scan), once per keyframe      -> vsc_push_scan
 *   :353  scManager.detectLoopClosureID(currentID), in ScanContextThread        -> vsc_detect
 * The stage the reference runs right after a hit, FastVGICP loop verification, is vilvgicp.h; detect -> verify is then on the device.
 * The database is resident: per entry the descriptor (float), the ring key (float), the sector key and the column norms (double).  Per
 * keyframe only the scan goes up, per detection only a vsc_result comes back.
 *
 * STAYS ON THE HOST (out of scope here):
 *   - the caller's checks on the result: historyID != 0 and the floor test (:357), keyframe selection (the pose graph is include/vilpgo.h);
 *   - the kd-tree's rebuild schedule (TREE_MAKING_PERIOD_ = 30, Scancontext.cpp:356-368): the reference searches a tree that is up to
 *     29 keyframes stale.  This library has no tree; a caller who wants that behaviour passes the stale tree's size as n_search.
 *
 * ARITHMETIC CONTRACT.  Unfused IEEE arithmetic in the order written; every sum runs in ascending index order.
 *   1 descriptor (makeScancontext, :153-197) per point [x y z intensity], in float: z' = float(double(z) + lidar_height), range =
 *                sqrtf(x*x + y*y), theta = float(xy2theta): the four branches of :25-38 evaluated in double on atan(double(y / x)) with
 *                the FLOAT quotient, (180.0 / M_PI) * atan(..), then 180 - .., 180 + .., 360 - ..  A point with double(range) >
 *                max_radius is skipped.  ring = clamp(int(ceil(double(range) / max_radius * 20)), 1, 20), sector =
 *                clamp(int(ceil(double(theta) / 360.0 * 60)), 1, 60); bin (ring - 1, sector - 1) keeps the maximum z'.  A bin starts at
 *                -1000 and a bin that ends at exactly -1000 becomes 0 (so does a bin whose points all lie below -1000, as in the
 *                reference).  Descriptor values are floats; they are stored as floats and widened to double when scoring.
 *                A NaN z' never wins a comparison, as in the reference.
 *                DEVIATION: a point with a non-finite x or y, or with x = y = 0, is dropped (the reference casts NaN to int there).
 *                DEVIATION: the maximum is order-independent; between -0 and +0 (equal in the reference, where the first stays) +0 wins.
 *   2 keys       (:200-229) ring key r: (sum over the 60 sectors in double) / 60, rounded to float (eig2stdvec's cast, the kd-tree's
 *                element type).  Sector key c: (sum over the 20 rings in double) / 20, double.  Column norm c: sqrt of the sum of squares
 *                over the 20 rings, double.  DEVIATION: Eigen's vectorised reductions sum in a build-dependent order; here ascending.
 *   3 candidates (VSC_MODE_REFERENCE, :374-382) squared L2 distance of the float ring keys, acc = acc + d*d in float over rings 0..19;
 *                the min(num_candidates, n_search) nearest entries of [0, n_search) ordered by (distance, index); a NaN distance orders
 *                last.  The search is exact.  DEVIATION: nanoflann may order equal distances differently and sums in blocks of four; with
 *                fewer entries than num_candidates the reference scores entry 0 again for each missing one, which cannot change its result.
 *   4 pair       (distanceBtnScanContext :118-150, distDirectSC :71-92) shift s: column j of the shifted entry is column (j - s) mod 60
 *                of the entry.  A column pair is skipped when either norm is 0; otherwise sim = dot / (nq * nd) with dot the sum over
 *                the 20 rings, summed over the query's columns j = 0..59; dist = 1.0 - sum / count (count = 0: NaN, never wins a strict <).
 *                REFERENCE mode: a = fastAlignUsingVkey (:95-115): per shift sqrt of the sum over j of (vq[j] - vd[(j - s) mod 60])^2,
 *                strict < from 10000000, the first minimum wins; then the shifts within R = int(round(0.5 * search_ratio * 60)) of a
 *                (circularly) are scored, visited in ascending shift order with strict < from 10000000, argmin 0.
 *                EXHAUSTIVE mode: all 60 shifts, same visiting rule.  One (query, entry, shift) triple gives the same bits in both modes.
 *   5 decision   (:338-430) entries are visited in candidate order (REFERENCE) or ascending index (EXHAUSTIVE), strict < from min_dist =
 *                10000000 with nn_idx = nn_align = 0; loop_id = nn_idx when min_dist < dist_thres, else -1; yaw_diff_rad =
 *                float(double(float(nn_align * 6.0)) * M_PI / 180.0).  With fewer than num_exclude_recent + 1 entries: loop_id -1, yaw 0,
 *                n_searched 0, nothing is submitted (:349-353).
 * SIGN OF nn_align.  Sector indices grow with the azimuth atan2(y, x) in the sensor frame.  A sensor that has turned by +psi about z
 * sees the world turned by -psi, so what the entry has in column c the query has in column c - psi / 6 deg.  Step 4 matches query column j
 * with entry column j - s, hence s = -psi / 6 deg (mod 60):  yaw(query) - yaw(entry) = -nn_align * 6 deg (mod 360, to the sector's width),
 * and the transform that takes query-frame points into the entry's frame starts from Rz(-yaw_diff_rad).
 * Results are bit-reproducible against tests/scancontext_ref.py wherever atan's last bits do not move a point across a sector edge.
 * Plain C, POD only, host pointers.  Needs a HIP device; there is no CPU fallback. */
#ifndef VILSC_H
#define VILSC_H
#include <stdint.h>
#include "vilsolve.h"
#ifdef __cplusplus
extern "C" {
#endif

#define VSC_NUM_RING 20            /* PC_NUM_RING */
#define VSC_NUM_SECTOR 60          /* PC_NUM_SECTOR */
#define VSC_MAX_CANDIDATES 16
#define VSC_NUM_KERNELS 6
#define VSC_MODE_REFERENCE 0       /* ring-key candidates, sector-key pre-alignment, +-R shifts: SCManager::detectLoopClosureID */
#define VSC_MODE_EXHAUSTIVE 1      /* every searched entry, all 60 shifts: the search of the original paper */

typedef struct vsc_ctx vsc_ctx;

typedef struct vsc_config {
    double lidar_height;           /* LIDAR_HEIGHT 2.0 */
    double max_radius;             /* PC_MAX_RADIUS 80.0; > 0 */
    double dist_thres;             /* SC_DIST_THRES 0.5 */
    double search_ratio;           /* SEARCH_RATIO 0.1; in [0, 1] */
    int32_t num_exclude_recent;    /* NUM_EXCLUDE_RECENT 5; >= 0 */
    int32_t num_candidates;        /* NUM_CANDIDATES_FROM_TREE 3; 1 .. VSC_MAX_CANDIDATES */
} vsc_config;

typedef struct vsc_result {
    double min_dist;               /* 10000000 when nothing won */
    int32_t loop_id;               /* nn_idx when min_dist < dist_thres, else -1 */
    int32_t nn_idx, nn_align;      /* the best entry and its column shift, whether or not it passed the threshold */
    int32_t n_searched;            /* entries [0, n_searched) were searched; 0 after the early return */
    float yaw_diff_rad;
    int32_t pad;
} vsc_result;

void vsc_default_config(vsc_config* cfg);
/* All device and pinned memory is allocated here.  cfg NULL: the defaults.  VIL_ERR_DEVICE without a HIP device,
 * VIL_ERR_INVALID_ARGUMENT for a size < 1 or a configuration outside the ranges above. */
int vsc_create(int32_t device, int32_t max_entries, int32_t max_points, const vsc_config* cfg, vsc_ctx** out);
void vsc_destroy(vsc_ctx* ctx);
/* makeAndSaveScancontextAndKeys: steps 1 and 2 for n points [x y z intensity] (n = 0 gives the all-zero descriptor), appended as entry
 * *id_out = the count before the call.  One submission, nothing is read back.  VIL_ERR_INVALID_ARGUMENT when n > max_points or the
 * database is full; nothing changes then. */
int vsc_push_scan(vsc_ctx* ctx, int32_t n, const float* xyzi, int32_t* id_out);
/* saveScancontextAndKeys for a float-valued descriptor, 20 x 60 row-major (ring, sector): step 2 only. */
int vsc_push_descriptor(vsc_ctx* ctx, const float* desc_20x60_rowmajor, int32_t* id_out);
/* detectLoopClosureID: the query is the newest entry, entries [0, n_search) are searched; n_search < 0: count - num_exclude_recent.
 * VIL_ERR_INVALID_ARGUMENT for n_search = 0 or > count, or an unknown mode.  One submission, one read-back (the record). */
int vsc_detect(vsc_ctx* ctx, int32_t mode, int32_t n_search, vsc_result* out);
int vsc_count(vsc_ctx* ctx);       /* entries, or VIL_ERR_INVALID_ARGUMENT */
int vsc_reset(vsc_ctx* ctx);       /* empties the database */
/* test hook: one entry; desc 1200 floats, ringkey20 20 floats, sectorkey60 60 doubles, each may be NULL */
int vsc_read_entry(vsc_ctx* ctx, int32_t id, float* desc, float* ringkey20, double* sectorkey60);
/* test hook: the scored entries of the last vsc_detect in the order step 5 visited them: min(num_candidates, n_searched) of them in
 * REFERENCE mode (candidates = their indices in (distance, index) order), n_searched in EXHAUSTIVE mode (candidates = 0, 1, 2, ..), none
 * after the early return.  dist / shift: step 4's result per scored entry.  VIL_ERR_INVALID_ARGUMENT when `capacity` is less than
 * their number.  Each pointer may be NULL. */
int vsc_debug_read(vsc_ctx* ctx, int32_t capacity, double* dist, int32_t* shift, int32_t* candidates);
/* measurement hook, as vdepth_profile_*: HIP events around the kernels; read returns launch counts and total durations of
 * {k_sc_bin, k_sc_finish, k_sc_cand, k_sc_select, k_sc_score, k_sc_decide} and resets them */
int vsc_profile_enable(vsc_ctx* ctx, int32_t enable);
int vsc_profile_read(vsc_ctx* ctx, int64_t* launches6, double* total_ms6);

#ifdef __cplusplus
}
#endif
#endif
