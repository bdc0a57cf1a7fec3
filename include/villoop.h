/* villoop.h -- C-ABI of the alignment fitness score and the loop-closure verification built on it: the number the reference reads after
 * every scan-to-scan alignment, pcl::Registration::getFitnessScore(), and the decisions it takes with it.
 *
 * Where the reference uses the score:
 *   vils_estimator/src/estimator.cpp:303          fitness_core = gicp->getFitnessScore(); it selects constraint_mode (:340-353) and scales
 *                                                 lidar_sqrt_info (:417).  The stateless part of that is include/vilicp_shim.hpp.
 *   lidar_mapping/src/globalMappingIkdTree.cpp
 *     :363-394  performSC_ICP                     the Scan Context candidate is kept when fitness < max_tolerable_fitness     -> vloop_verify, n_cand = 1
 *     :434-510  findLoopClosure                   every proximity candidate is aligned and scored, the smallest score wins  -> vloop_verify
 *     :512-573  performICP                        FastVGICP align, hasConverged, getFitnessScore, poseUpdate.inv()           -> vloop_verify, per candidate
 *     :600-638  updateLocalization                the same align-then-score pair                                             -> vgicp_align + vloop_score
 *   lidar_mapping/src/globalMappingOcTree.cpp:388-410, :463-540, :541-600 hold the same code.
 *   max_tolerable_fitness is a global of the node: 1.0 in include/global_mapping/util.h:86, set to 2.0 in globalMappingOcTree.cpp:1004.
 *   The caller passes its value in vloop_options.
 *
 * PCL is not part of the reference tree.  The semantics of getFitnessScore(max_range) below are restated from PCL's documented
 * behaviour (registration.hpp: the source is transformed by final_transformation_, each transformed point asks the target's search
 * tree for its nearest neighbour, squared distances not above max_range are averaged); they are not transcribed from its source.
 *
 * ARITHMETIC CONTRACT of vloop_score, per transform T (row-major 4x4 double, source -> target; only its first three rows are read):
 *   1 T is rounded to float: final_transformation_ is a Matrix4f.
 *   2 every source point (x, y, z) is transformed in unfused float: q_r = ((m_r0 * x + m_r1 * y) + m_r2 * z) + m_r3 for r = 0, 1, 2.
 *   3 its nearest target point is the minimum over ALL target points of (d2, index) in lexicographic order, d2 the unfused float
 *     (dx * dx + dy * dy) + dz * dz with dx = q_x - t_x, ...  The search is exact; equal distances go to the smaller target index.
 *     DEVIATION: PCL's kd-tree (FLANN) sums the squares in its own order and breaks ties by its traversal.
 *   4 a point is used when (double)d2 <= max_range.  As in PCL, max_range is compared with the SQUARED distance (a caller that means
 *     2 m passes 4.0).  getFitnessScore()'s default, the largest double, uses every point.
 *   5 score = (sum of the used d2, in double) / n_used; n_used = 0 gives DBL_MAX.
 *     The sum has one order: the source points are cut into blocks of VLOOP_SUM_BLOCK = 256 consecutive points; a block's partial is the
 *     sequential sum of its used d2 in ascending point order starting from 0.0; the total is the sequential sum of the partials in
 *     ascending block order starting from 0.0.  It does not depend on the search path, the grid or the scheduling; no floating-point
 *     atomics are used.  DEVIATION: PCL adds the points one by one.
 * Both search paths (uniform grid, exhaustive) return the same bits.  tests/loopverify_ref.py restates 1-5 in NumPy.
 * Coordinates are assumed to stay below 2^31 grid cells in magnitude.
 *
 * vloop_verify is performICP over a list of candidates plus the selection of findLoopClosure.  OUT OF SCOPE, left with the caller:
 *   - the skip_recent_poses, proximity_threshold and floor filters (:449-465): host bookkeeping over the pose table;
 *   - the two pcl::ApproximateVoxelGrid calls of performICP (:521-527): the caller passes the filtered clouds;
 *   - what is done with the winner.  The pose graph itself is include/vilpgo.h: best.delta and best.fitness go into vpgo_add_between as they
 *     are (:387, :498), and vpgo_relative gives the next candidate's guess (:370).
 * DEVIATION: delta is the inverse of the float-rounded result in double, (R^-1, -R^-1 t) with the 3 x 3 inverse by cofactors, so that
 * delta T is the identity to double rounding.  For an orthonormal R that is (R^T, -R^T t); the float-rounded R is orthonormal to 6e-8
 * only.  The reference goes through its own Quaternion / Pose6D types (:569-570), which renormalise the rotation instead.
 * Plain C, POD only, host pointers.  Needs a HIP device; there is no CPU fallback. */
#ifndef VILLOOP_H
#define VILLOOP_H
#include <stdint.h>
#include "vilsolve.h"
#include "vilvgicp.h"
#ifdef __cplusplus
extern "C" {
#endif

#define VLOOP_NUM_KERNELS 4
#define VLOOP_MAX_BATCH 16         /* transforms per vloop_score: the per-point outputs of a batch are laid out at create */
#define VLOOP_SUM_BLOCK 256        /* step 5 */

typedef struct vloop_ctx vloop_ctx;

typedef struct vloop_candidate {
    int32_t n;                     /* 1 .. max_points */
    int32_t pad;
    const float* xyz;              /* n x 3, the candidate keyframe's (filtered) scan: the alignment's target */
    double guess[16];              /* pose2.inv() * pose1, row-major 4x4, query -> candidate; rounded to float before use (:555-557) */
} vloop_candidate;

typedef struct vloop_options {
    vgicp_options reg;             /* vgicp_default_options: FastVGICP as performICP configures it */
    double resolution;             /* setResolution(0.5), :535 */
    float max_tolerable_fitness;   /* the running minimum starts here (:443); a candidate must be strictly below it (:379, :477) */
    int32_t pad;
} vloop_options;

typedef struct vloop_candidate_result {
    int32_t converged;             /* hasConverged(); 0: the candidate is skipped (:560), fitness = FLT_MAX, n_used = 0 */
    float fitness;                 /* (float)getFitnessScore(), :564 */
    int32_t n_used;
    int32_t iterations;            /* vgicp_summary.iterations */
    double T[16];                  /* getFinalTransformation(): the alignment's result rounded to float, query -> candidate */
} vloop_candidate_result;

typedef struct vloop_best {
    int32_t index;                 /* the winning candidate, -1: none */
    float fitness;                 /* the winner's; max_tolerable_fitness when there is none */
    int32_t n_used;
    int32_t pad;
    double T[16];                  /* the winner's vloop_candidate_result.T; the identity when there is none */
    double delta[16];              /* its inverse: poseUpdate.inv(), :569-570 */
} vloop_best;

/* All device and pinned memory for clouds of up to max_points points is allocated here; only the search grid's work space grows on
 * demand.  VIL_ERR_INVALID_ARGUMENT for max_points <= 0 or out = NULL (checked first), VIL_ERR_DEVICE without a HIP device. */
int vloop_create(int32_t device, int32_t max_points, vloop_ctx** out);
void vloop_destroy(vloop_ctx* ctx);
void vloop_default_options(vloop_options* o);      /* vgicp_default_options, resolution 0.5, max_tolerable_fitness 1.0 (util.h:86) */
/* The cloud (float xyz, stride 3, n >= 1) goes up and stays resident; set_target also builds the search grid when the cloud is large
 * enough for it.  VIL_ERR_NON_FINITE for a non-finite coordinate, VIL_ERR_INVALID_ARGUMENT for n < 1 or n > max_points; the resident
 * cloud is unchanged then. */
int vloop_set_target(vloop_ctx* ctx, int32_t n, const float* xyz);
int vloop_set_source(vloop_ctx* ctx, int32_t n, const float* xyz);
/* Targets of at least min_points points (default 1024) are searched through a uniform grid of cell edge `cell` metres (default 0.5,
 * used as given), smaller ones exhaustively.  Takes effect at the next vloop_score. */
int vloop_set_grid(vloop_ctx* ctx, int32_t min_points, double cell);
/* getFitnessScore(max_range) of the resident pair at n_T transforms (1 .. VLOOP_MAX_BATCH), T16s = n_T x 16 doubles: one submission,
 * one read-back of n_T records.  scores: n_T doubles; n_used: n_T counts, may be NULL.  nn_d2 / nn_idx: debug outputs, n_T x n_source
 * each (step 3's distance and target index per source point), may be NULL; they are copied in the same submission.
 * VIL_ERR_INVALID_ARGUMENT without a resident pair or for a NaN max_range, VIL_ERR_NON_FINITE for a non-finite entry of T. */
int vloop_score(vloop_ctx* ctx, int32_t n_T, const double* T16s, double max_range, double* scores, int32_t* n_used, float* nn_d2, int32_t* nn_idx);
/* The query scan against n_cand >= 0 candidates in the given order.  The query becomes vloop's resident source and reg's source
 * (uploaded once each); per candidate: vgicp_set_target(reg, candidate, NULL, resolution), vloop_set_target, vgicp_align from the
 * float-rounded guess, and, when it converged, fitness = (float)vloop_score(T, max_range = DBL_MAX).  The winner is the first candidate
 * whose fitness is strictly below the running minimum, which starts at max_tolerable_fitness: of two equal candidates the earlier one
 * wins.  per_candidate: n_cand records, may be NULL.  Sizes are checked for every candidate before anything is submitted. */
int vloop_verify(vloop_ctx* ctx, vgicp_ctx* reg, int32_t n_query, const float* query_xyz, int32_t n_cand, const vloop_candidate* candidates, const vloop_options* options,
                 vloop_best* best, vloop_candidate_result* per_candidate);
/* measurement hook, as vsc_profile_*: HIP events around the kernels of vloop_score; read returns launch counts and total durations of
 * {k_loop_grid, k_loop_brute, k_loop_sum, k_loop_finish} and resets them */
int vloop_profile_enable(vloop_ctx* ctx, int32_t enable);
int vloop_profile_read(vloop_ctx* ctx, int64_t* launches4, double* total_ms4);

#ifdef __cplusplus
}
#endif
#endif
