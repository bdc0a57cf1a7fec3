/* vilepi.h -- C-ABI of the epipolar outlier rejection and the undistortion of tracked points of mVIL-Fusion's feature tracker: the two
 * steps between vtrack_track (viltrack.h) and vdepth_register (vildepth.h).
 *
 * Replaces FeatureTracker::rejectWithF (feature_tracker_/src/feature_tracker.cpp:169-202: both point sets lifted through the camera model
 * into a virtual pinhole camera, cv::findFundamentalMat(FM_RANSAC, F_THRESHOLD, 0.99), the status vector) and
 * FeatureTracker::undistortedPoints (:258-306: the lifted points and their velocities against the previous image's table of ids), with
 * PinholeCamera::liftProjective / distortion (camera_model/src/camera_models/PinholeCamera.cc:450-510, :646-662).
 *
 * OpenCV and camodocal are not on the machines this was written on, so this is a RESTATEMENT WITH A WRITTEN CONTRACT, as viltrack.h is.
 * A RANSAC whose hypothesis h depends on (seed, h) alone can evaluate its hypotheses in parallel and still return exactly what the
 * sequential loop with its adaptive stop returns: the device evaluates, the host replays the loop over the counts.  tests/epipolar_ref.py
 * transcribes this header.
 *
 * DEVIATIONS from the reference, all of vepi_reject:
 *   - the minimal sample is 8 points with one solution (the normalised 8-point fit).  OpenCV's FM_RANSAC draws 7 and solves a cubic whose
 *     roots go through acos / cos.  The reference never runs RANSAC on fewer than 8 points anyway (:171).
 *   - the generator is the counter-based one of step 3, not cv::RNG.
 *   - when no hypothesis reaches 8 inliers the reference is left with an empty status and reads past it; here status is all 1,
 *     best_hypothesis = -1, found = 0 and the call returns VIL_OK (step 7).
 * STAYS ON THE HOST: reduceVector on `status`, the ids / track_cnt bookkeeping (both on the device in vfeat_read_image, vilfeat.h, which
 * runs the kernels of this row on resident points), the other camodocal models (VIL_ERR_UNSUPPORTED).
 *
 * ARITHMETIC CONTRACT.  f64 is unfused IEEE double in the order written (a op b op c is (a op b) op c); f32(x) rounds to nearest even.
 *   1 lift        inv_K11 = 1/fx, inv_K13 = -cx/fx, inv_K22 = 1/fy, inv_K23 = -cy/fy (computed once, on the host).  For a pixel (u, v) given
 *                 as float32 and widened: m_d = (inv_K11 u + inv_K13, inv_K22 v + inv_K23).  d(x, y): mx2 = x x, my2 = y y, mxy = x y,
 *                 rho2 = mx2 + my2, rad = k1 rho2 + k2 rho2 rho2; d = (x rad + 2.0 p1 mxy + p2 (rho2 + 2.0 mx2), y rad + 2.0 p2 mxy +
 *                 p1 (rho2 + 2.0 my2)).  m_u = m_d - d(m_d), then VEPI_LIFT_STEPS - 1 = 7 times more m_u = m_d - d(m_u).  With k1 = k2 =
 *                 p1 = p2 = 0, m_u = m_d, which is ((u - cx) / fx, (v - cy) / fy) to 1 ulp OF THE LARGER TERM, max(u, cx) / fx: the two
 *                 terms cancel towards the principal point, where an ulp of the result means nothing.  The eight steps are the reference's and do NOT converge at the corners of its camera
 *                 (config/mynteye_leishen_indoor.yaml:13-22): projecting lift(p) back misses p by up to 0.0527 px (per coordinate) over the central
 *                 400 x 300 pixels and by up to 0.2367 px over the whole 640 x 480 (tests/test_epipolar_ref.py).  Not to be "fixed".
 *   2 virtual     p = (f32(focal m_u.x + width / 2.0), f32(focal m_u.y + height / 2.0)) for both point sets; p1 of cur, p2 of forw.
 *   3 sample      mix(x): z = x + 0x9E3779B97F4A7C15; z = (z ^ z >> 30) 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) 0x94D049BB133111EB; z ^ z >> 31,
 *                 all modulo 2^64.  Hypothesis h draws r_k = mix((seed ^ h 0xD1342543DE82EF95) + k) for k = 0, 1, ...; index
 *                 ((r_k >> 32) n) >> 32; an index already in the sample is dropped and the next k is drawn, until there are 8.  Nothing else
 *                 enters the sample.  After 65536 draws without 8 distinct indices the missing ones are 0 and the hypothesis has no model (at
 *                 n = 8 a chance of (7/8)^65000).
 *   4 model       per image, over the 8 sampled points in sample order: c = (sum x / 8.0, sum y / 8.0); mean = (sum sqrt(dx dx + dy dy)) / 8.0
 *                 with (dx, dy) = (x, y) - c; no model unless mean > 0; s = sqrt(2.0) / mean; (u, v) = ((x - c.x) s, (y - c.y) s).
 *                 Row r = [u2 u1, u2 v1, u2, v2 u1, v2 v1, v2, u1, v1, 1]; A[i][j] = sum_r row_r[i] row_r[j] in sample order, 9 x 9.
 *                 jacobi(A), N x N, V = I: VEPI_JACOBI_SWEEPS = 10 sweeps over (p, q), p < q in row order; skipped when A[p][q] == 0;
 *                 theta = (A[q][q] - A[p][p]) / (2.0 A[p][q]); t = (theta >= 0 ? 1.0 : -1.0) / (|theta| + sqrt(theta theta + 1.0));
 *                 c = 1.0 / sqrt(t t + 1.0); s = t c; for k != p, q: (A[k][p], A[k][q]) = (c A[k][p] - s A[k][q], s A[k][p] + c A[k][q])
 *                 from the old pair, mirrored into A[p][k], A[q][k]; A[p][p] -= t A[p][q]; A[q][q] += t A[p][q]; A[p][q] = A[q][p] = 0;
 *                 for every k: (V[k][p], V[k][q]) = (c V[k][p] - s V[k][q], s V[k][p] + c V[k][q]).  Ten sweeps leave a relative
 *                 off-diagonal of 2e-16 or less (eight already do).  The smallest eigenvector is the column of V at the smallest diagonal
 *                 entry, the lowest index among equal ones.
 *                 Fn = that column of jacobi(A), row-major 3 x 3.  M[i][j] = (Fn[0][i] Fn[0][j] + Fn[1][i] Fn[1][j]) + Fn[2][i] Fn[2][j];
 *                 v = smallest eigenvector of jacobi(M); w[i] = (Fn[i][0] v[0] + Fn[i][1] v[1]) + Fn[i][2] v[2]; Fn[i][j] -= w[i] v[j]
 *                 (rank 2).  With t1 = (-(s1 c1.x), -(s1 c1.y)) and t2 alike: G[i] = [Fn[i][0] s1, Fn[i][1] s1, (Fn[i][0] t1.x + Fn[i][1]
 *                 t1.y) + Fn[i][2]]; F[0] = G[0] s2, F[1] = G[1] s2, F[2][j] = (G[0][j] t2.x + G[1][j] t2.y) + G[2][j]  (F = T2^T Fn T1,
 *                 p2^T F p1 = 0).  A non-finite entry of F gives no model.  A hypothesis without a model has count 0.
 *   5 score       per point, coordinates widened to f64: a = (F[0][0] x1 + F[0][1] y1) + F[0][2], b, c from rows 1, 2 alike;
 *                 e2 = (d d) (1.0 / (a a + b b)) with d = (x2 a + y2 b) + c.  Then a = (F[0][0] x2 + F[1][0] y2) + F[2][0], b, c from
 *                 columns 1, 2 alike; e1 = (d d) (1.0 / (a a + b b)) with d = (x1 a + y1 b) + c.  Inlier iff e1 <= thr thr and e2 <= thr thr
 *                 (the larger of the two distances; false for NaN).  The margin of the pair is |err / (thr thr) - 1.0| with err = e1 > e2 ?
 *                 e1 : e2; a NaN margin is ignored.
 *   6 loop        on the host, in double with the C library's log / pow, from the counts: niters = max_iters, best = 0; for h = 0, 1, ...
 *                 while h < niters: when count_h > max(best, 7): best = count_h, the best hypothesis is h, niters = min(niters, N) with
 *                 ratio = (n - count_h) / (double)n, den = 1.0 - pow(1.0 - ratio, 8); N = 0 when den < DBL_MIN; else num = log(1.0 -
 *                 confidence), den = log(den), N = max_iters when den >= 0 or -num >= max_iters * -den, else N = (int)rint(num / den).
 *                 THE RESULT OF THE CALL IS WHAT THIS LOOP RETURNS: the inlier flags of the best hypothesis, its index, its count and the
 *                 number of hypotheses the loop consumed (h at its end) -- whatever cfg.batch is.
 *   7 no model    no hypothesis reached 8 inliers: status all 1, best_hypothesis = -1, found = 0, VIL_OK.
 *   8 undistort   un = (f32(m_u.x), f32(m_u.y)) (the reference divides by z = 1.0).  vel = (f32((f64(un.x) - f64(prev.x)) / dt), the same in
 *                 y) when ids[i] != -1 and ids[i] occurs in the previous call's table, prev being the un of its FIRST occurrence in that
 *                 call's order (std::map::insert keeps the first); otherwise vel = (0, 0) -- on the first call and after vepi_reset for
 *                 every point.  dt == 0 gives what IEEE gives.  This call's (ids, un) then replace the table.
 * Plain C, POD only, host pointers.  Needs a HIP device; there is no CPU fallback. */
#ifndef VILEPI_H
#define VILEPI_H
#include <stdint.h>
#include "vilsolve.h"
#ifdef __cplusplus
extern "C" {
#endif

#define VEPI_NUM_KERNELS 3           /* k_epi_lift, k_epi_hyp, k_epi_undist */
#define VEPI_MIN_POINTS_LIMIT 8
#define VEPI_MAX_POINTS_LIMIT 4096   /* the previous table's ids are staged in LDS */
#define VEPI_MAX_ITERS_LIMIT 65536
#define VEPI_SAMPLE 8
#define VEPI_JACOBI_SWEEPS 10
#define VEPI_LIFT_STEPS 8

/* camera models of camodocal; only VEPI_MODEL_PINHOLE is taken, the others give VIL_ERR_UNSUPPORTED */
enum { VEPI_MODEL_PINHOLE = 0, VEPI_MODEL_CATA = 1, VEPI_MODEL_EQUIDISTANT = 2, VEPI_MODEL_SCARAMUZZA = 3 };
/* how the result of a vepi_reject comes back: the kernel writes the counts and the inlier rows into pinned host memory (the design that
 * was kept: 0.010 - 0.012 ms per call faster at one launch), or they stay in device memory and the counts of a batch and the winner's row are copied
 * (kept for tools/bench_epipolar.py, profiles/epipolar.txt; the result is the same) */
enum { VEPI_READBACK_PINNED = 0, VEPI_READBACK_COPY = 1 };
/* what vepi_debug_read returns, all of the last vepi_reject that launched */
enum { VEPI_DBG_CUR_PTS = 0, VEPI_DBG_FORW_PTS = 1, VEPI_DBG_SAMPLES = 2, VEPI_DBG_COUNTS = 3, VEPI_DBG_F = 4, VEPI_DBG_MARGINS = 5 };

typedef struct vepi_ctx vepi_ctx;

typedef struct vepi_cfg {
    double fx, fy, cx, cy, k1, k2, p1, p2;  /* PINHOLE of camodocal; fx, fy finite and not 0 */
    double focal;                           /* the virtual camera of rejectWithF; reference: FOCAL_LENGTH 460, COL, ROW */
    int32_t width, height;                  /* 1 .. 65536 each */
    int32_t model;                          /* VEPI_MODEL_* */
    int32_t max_points;                     /* VEPI_MIN_POINTS_LIMIT .. VEPI_MAX_POINTS_LIMIT */
    int32_t max_iters;                      /* 1 .. VEPI_MAX_ITERS_LIMIT; reference (OpenCV's default): 1000 */
    int32_t batch;                          /* hypotheses per launch, 1 .. max_iters; 0: max_iters */
    int32_t readback;                       /* VEPI_READBACK_*; 0 in a product.  The other value exists for tools/bench_epipolar.py only */
    int32_t reserved;
} vepi_cfg;

typedef struct vepi_summary {
    int32_t n_points, n_inliers;   /* points given; inliers of the best hypothesis (n_points when nothing was launched or found) */
    int32_t found;                 /* 1: a hypothesis reached 8 inliers */
    int32_t best_hypothesis;       /* its index, -1 without one */
    int32_t consumed;              /* hypotheses the loop of step 6 consumed */
    int32_t evaluated;             /* hypotheses the device evaluated: whole batches, each cut at what the loop still allowed when it was launched */
    int32_t launches;              /* launches of k_epi_hyp */
    int32_t reserved;
} vepi_summary;

/* All device and pinned memory is allocated here.  VIL_ERR_INVALID_ARGUMENT for a NULL pointer or a value outside the ranges above, then
 * VIL_ERR_UNSUPPORTED for another model than PINHOLE, then VIL_ERR_DEVICE without a HIP device. */
int vepi_create(int32_t device, const vepi_cfg* cfg, vepi_ctx** out);
void vepi_destroy(vepi_ctx* ctx);
/* rejectWithF.  cur_xy, forw_xy: n points [x y] each, in pixels of the real camera; status: n bytes, 1 = kept.  thr > 0 (reference:
 * F_THRESHOLD), 0 < confidence < 1 (reference: 0.99).  n < 8: status all 1, nothing is launched (:171).  Otherwise one upload, one
 * k_epi_lift, ceil(evaluated / batch) launches of k_epi_hyp with a synchronisation after each (VEPI_READBACK_COPY: and a copy of the counts;
 * then one of the winner's row).
 * VIL_ERR_INVALID_ARGUMENT for n < 0, n > max_points, a NULL pointer (with n > 0), thr or confidence outside their ranges (NaN included);
 * nothing is written then.  `out` may be NULL. */
int vepi_reject(vepi_ctx* ctx, int32_t n, const float* cur_xy, const float* forw_xy, double thr, double confidence, uint64_t seed, uint8_t* status, vepi_summary* out);
/* undistortedPoints (step 8).  xy: n points in pixels, ids: their ids (-1: none yet), dt: cur_time - prev_time.  un_xy, vel_xy: 2n floats
 * each.  n = 0 empties the table.  One upload, one launch, one read-back.  VIL_ERR_INVALID_ARGUMENT for n < 0, n > max_points or a NULL
 * pointer (with n > 0); nothing is written and the table stays. */
int vepi_undistort(vepi_ctx* ctx, int32_t n, const float* xy, const int32_t* ids, double dt, float* un_xy, float* vel_xy);
/* empties the table of vepi_undistort: the next call gives zero velocities */
int vepi_reset(vepi_ctx* ctx);
/* test hook, of the last vepi_reject with n >= 8.  _CUR_PTS / _FORW_PTS: step 2's points, n x 2 floats.  _SAMPLES: 8 int32 per evaluated
 * hypothesis; _COUNTS: one int32 each; _MARGINS: one double each, the minimum of step 5's margin over the points (inf without one).
 * _F: the 9 doubles of the best hypothesis' F (VIL_ERR_INVALID_ARGUMENT when found = 0).  VIL_ERR_INVALID_ARGUMENT when capacity_bytes is
 * too small or before such a call. */
int vepi_debug_read(vepi_ctx* ctx, int32_t what, void* dst, int64_t capacity_bytes);
/* measurement hook, as vtrack_profile_*: HIP events around the kernels; read returns the launch counts and total durations of the
 * VEPI_NUM_KERNELS kernels in the order listed above and resets them */
int vepi_profile_enable(vepi_ctx* ctx, int32_t enable);
int vepi_profile_read(vepi_ctx* ctx, int64_t* launches3, double* total_ms3);

#ifdef __cplusplus
}
#endif
#endif
