/* vilpgo.h -- C-ABI of the on-device pose-graph optimisation that closes the loop-closure path: vsc_* finds the candidate, vloop_verify
 * aligns and scores it, and its delta and fitness become a between factor of the graph optimised here.
 *
 * Where the reference keeps its graph (lidar_mapping/src/globalMappingIkdTree.cpp; globalMappingOcTree.cpp holds the same code):
 *   :153-159  PriorFactor<Pose3> on the first pose, Variances(1e-9 x 3, 1e-4 x 3)                       -> vpgo_add_prior
 *   :216-228  GPSFactor on the latest pose                                                               -> vpgo_add_position
 *   :259-270  BetweenFactor(k - 1, k) odometry, isam->update, calculateEstimate for every mapped scan    -> vpgo_add_pose, vpgo_add_between, vpgo_optimize
 *   :370      pose2.inv() * pose1, the guess of the alignment                                            -> vpgo_relative
 *   :379-390, :487-508  BetweenFactor(current, history) from the verified loop, one or two more updates  -> vpgo_add_between, vpgo_optimize
 * GTSAM is not part of the reference tree; what follows restates the documented behaviour of Pose3, BetweenFactor, PriorFactor, GPSFactor
 * and noiseModel::Diagonal::Variances, it is not transcribed from GTSAM's source.
 *
 * ARITHMETIC CONTRACT (all in double)
 *   State   N poses T_k = (R_k, t_k), keys 0 .. N-1 in the order they were added.  A step d = [dw; dv], rotation part first as in Pose3,
 *           is applied as t <- t + R dv, then R <- R Exp(dw), then R <- R (3 I - R^T R) / 2 (one Newton step towards the nearest
 *           orthonormal matrix: the fixed re-orthonormalisation; it is part of every candidate state).
 *   Noise   variances, as noiseModel::Diagonal::Variances: component k of a residual is divided by sqrt(var_k).
 *   Prior   on pose i, measurement Z:      r = [Log(Z_R^T R_i); Z_R^T (t_i - Z_t)]                              six variances
 *   Between (i, j, Z), D = Z^-1 T_i^-1 T_j: r = [Log(D_R); D_t], D_R = Z_R^T R_i^T R_j, D_t = Z_R^T (R_i^T (t_j - t_i) - Z_t)   six variances
 *           i > j is a normal case (the loop factors are (current, history)), i == j is invalid.
 *   Position on pose i, measurement z:     r = t_i - z                                                           three variances
 *   DEVIATION (chart): [Log(R); t] is Pose3's local chart with GTSAM_POSE3_EXPMAP off, the default of GTSAM 4.0.x.  A GTSAM built with the
 *           full SE(3) logarithm minimises a slightly different cost; the reference pins no GTSAM version (PARITY UNPINNED).
 *   Log     v = (R32 - R23, R13 - R31, R21 - R12) / 2, s = |v|, c = (trace R - 1) / 2, theta = atan2(s, c), Log(R) = k v with
 *           k = theta / s, and k = 1 + theta^2 / 6 + 7 theta^4 / 360 when theta < VPGO_SMALL_ANGLE.  Residual rotations up to pi - 0.1 rad
 *           are in contract; nearer to pi the same formula runs without a promise.
 *   Exp     R = I + a [w]x + b [w]x^2, theta = |w|, a = sin(theta) / theta, b = 2 sin^2(theta / 2) / theta^2; below VPGO_SMALL_ANGLE
 *           a = 1 - theta^2 / 6, b = 1 / 2 - theta^2 / 24.
 *   Jacobians  with w = Log(.), theta = |w|: Jri(w) = I + [w]x / 2 + e [w]x^2, e = 1 / theta^2 - (1 + cos theta) / (2 theta sin theta), and
 *           e = 1 / 12 + theta^2 / 720 below VPGO_SMALL_ANGLE.  Prior: dr/dd_i = [Jri, 0; 0, Z_R^T R_i].  Position: [0, R_i].
 *           Between: dr/dd_j = [Jri, 0; 0, D_R], dr/dd_i = [-Jri R_j^T R_i, 0; Z_R^T [p]x, -Z_R^T], p = R_i^T (t_j - t_i).
 *   Cost    1/2 sum |r|^2 over the whitened residuals.  The sum has one order: blocks of VPGO_SUM_BLOCK = 256 consecutive factors in factor
 *           order, a block summed sequentially from 0.0, the partials summed sequentially from 0.0 (the scheme of VLOOP_SUM_BLOCK).
 *           A pose's diagonal block of J^T J and its gradient J^T r are the sums of its factors' contributions in ascending factor index,
 *           gathered through an adjacency table.  No floating-point atomics anywhere: results are bit-identical from run to run and from
 *           process to process, and do not depend on how the graph was appended.
 *   Minimiser  Levenberg-Marquardt on H = J^T J + lambda I with the gain ratio rho = (cost - cost') / (d^T (lambda d - g) / 2) and Nielsen's
 *           update: accepted (rho > 0, cost' finite): lambda *= max(1/3, 1 - (2 rho - 1)^3), nu = 2; rejected (or H not positive definite):
 *           lambda = max(lambda nu, VPGO_LAMBDA_FLOOR), nu *= 2.  Every attempt counts as an iteration.  It stops on the first of
 *           max |d| < step_tolerance, an accepted relative cost decrease < cost_tolerance, max_iterations.  initial_lambda = 0 is allowed
 *           and makes the first step a pure Gauss-Newton step.
 *           This is the fixed point that iSAM2 with relinearizeThreshold = 0.01 approximates; it is NOT iSAM2's trajectory of intermediate
 *           estimates (no Bayes tree, no partial relinearisation).
 *   Solve   one level of nested dissection.  Separators: every key k with (k + 1) % VPGO_SEGMENT == 0, and both endpoints of every between
 *           factor with |i - j| > 1.  The keys between two separators form a chain segment that is factorised by block Cholesky with its (at
 *           most two) boundary couplings carried as right-hand-side columns; the Schur complement on the separators is dense, at most
 *           6 VPGO_MAX_SEPARATORS wide, and factorised by a blocked fp64 Cholesky on the matrix cores.
 * tests/posegraph_ref.py restates the contract in NumPy.
 * OUT OF SCOPE, left with the caller: iSAM2's intermediate estimates, robust kernels (the reference uses none), the map regeneration from the
 * corrected poses (:306-310) and the floor / key bookkeeping around the graph.
 * Plain C, POD only, host pointers.  Needs a HIP device; there is no CPU fallback. */
#ifndef VILPGO_H
#define VILPGO_H
#include <stdint.h>
#include "vilsolve.h"
#ifdef __cplusplus
extern "C" {
#endif

#define VPGO_NUM_KERNELS 11
#define VPGO_SEGMENT 64              /* a segment's working set is 19 columns x 6 doubles per wave and one trip per key: 63 dependent 6 x 6 steps */
#define VPGO_MAX_SEPARATORS 256      /* the dense reduced system is at most 1536 wide (two 19 MB arrays, allocated at create) */
#define VPGO_SUM_BLOCK 256
#define VPGO_SMALL_ANGLE 1e-4
#define VPGO_LAMBDA_FLOOR 1e-6

#define VPGO_PRIOR 0
#define VPGO_BETWEEN 1
#define VPGO_POSITION 2

#define VPGO_TERM_NONE 0             /* nothing to optimise: no pose or no factor */
#define VPGO_TERM_STEP 1
#define VPGO_TERM_COST 2
#define VPGO_TERM_MAX_ITERATIONS 3

typedef struct vpgo_ctx vpgo_ctx;

typedef struct vpgo_options {
    int32_t max_iterations;          /* 20; 1 .. VPGO_MAX_ITERATIONS */
    int32_t pad;
    double initial_lambda;           /* 1e-5, GTSAM's lambdaInitial; >= 0 */
    double step_tolerance;           /* 1e-10 */
    double cost_tolerance;           /* 1e-12 */
} vpgo_options;
#define VPGO_MAX_ITERATIONS 100

typedef struct vpgo_summary {
    int32_t iterations;              /* attempts, accepted or not */
    int32_t accepted;
    int32_t termination;             /* VPGO_TERM_* */
    int32_t reduced_size;            /* 6 x separators: the width of the dense reduced system */
    int32_t n_separators;
    int32_t n_segments;
    double initial_cost;
    double final_cost;
    double final_lambda;
} vpgo_summary;

/* All device and pinned memory is allocated here.  VIL_ERR_INVALID_ARGUMENT for max_poses <= 0, max_factors <= 0 or out = NULL (checked
 * first), VIL_ERR_DEVICE without a HIP device. */
int vpgo_create(int32_t device, int32_t max_poses, int32_t max_factors, vpgo_ctx** out);
void vpgo_destroy(vpgo_ctx* ctx);
void vpgo_default_options(vpgo_options* o);
/* The graph is resident and grows by appending; an append uploads the new pose or factor only.  Poses and measurements are row-major 4 x 4
 * doubles (the first three rows are read).  VIL_ERR_NON_FINITE for a non-finite entry, VIL_ERR_INVALID_ARGUMENT for a key out of range,
 * i == j, or a variance that is not finite and positive, VIL_ERR_CAPACITY when max_poses, max_factors or VPGO_MAX_SEPARATORS would be
 * exceeded (a graph that cannot be solved is refused where it is built, not at vpgo_optimize).  The graph is unchanged after any error. */
int vpgo_add_pose(vpgo_ctx* ctx, const double* T16, int32_t* key);
int vpgo_add_prior(vpgo_ctx* ctx, int32_t i, const double* Z16, const double* var6);
int vpgo_add_between(vpgo_ctx* ctx, int32_t i, int32_t j, const double* Z16, const double* var6);
int vpgo_add_position(vpgo_ctx* ctx, int32_t i, const double* z3, const double* var3);
int vpgo_size(vpgo_ctx* ctx, int32_t* n_poses, int32_t* n_factors, int32_t* n_separators);
/* The whole Levenberg-Marquardt loop is one enqueued sequence of launches; the device sets a finished flag and the launches that remain
 * return at once.  One read-back: the summary, through pinned memory. */
int vpgo_optimize(vpgo_ctx* ctx, const vpgo_options* options, vpgo_summary* summary);
int vpgo_get_poses(vpgo_ctx* ctx, int32_t first, int32_t n, double* T16s);
/* T_j^-1 T_i: the guess of vloop_candidate for query i against candidate j (:370) */
int vpgo_relative(vpgo_ctx* ctx, int32_t i, int32_t j, double* T16);
/* debug output at the current state.  r: n_factors x 6 whitened residuals (a position factor fills three, the rest is 0); J_i, J_j:
 * n_factors x 6 x 6 row-major whitened Jacobians with respect to the factor's first and second pose (J_j is 0 for unary factors);
 * cost: one double; g: n_poses x 6, J^T r.  Any of them may be NULL. */
int vpgo_eval(vpgo_ctx* ctx, double* r, double* J_i, double* J_j, double* cost, double* g);
/* debug output: d (n_poses x 6), the step the last attempt of the last vpgo_optimize solved for, as the device holds it.  The tests judge the
 * linear solve on it: the difference of the states before and after carries the rounding of the 20 m coordinates it was added to. */
int vpgo_get_step(vpgo_ctx* ctx, double* d);
/* measurement hook, as vloop_profile_*: launch counts and total durations of {k_pgo_lin, k_pgo_gather, k_pgo_segment, k_pgo_schur,
 * k_pgo_chol, k_pgo_dense_back, k_pgo_seg_back, k_pgo_update, k_pgo_reduce, k_pgo_decide, k_pgo_finish} of the last vpgo_optimize */
int vpgo_profile_enable(vpgo_ctx* ctx, int32_t enable);
int vpgo_profile_read(vpgo_ctx* ctx, int64_t* launches11, double* total_ms11);

#ifdef __cplusplus
}
#endif
#endif
