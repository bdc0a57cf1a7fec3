/* viltrack.h -- C-ABI of the KLT visual front end of mVIL-Fusion's feature tracker: camera images in, tracked points, setMask's
 * decisions and new corners out.  These are the points vdepth_register decorates, vilformat.hpp serialises and vil_win_push_frame consumes.
 *
 * Replaces, inside FeatureTracker::readImage (feature_tracker_/src/feature_tracker.cpp:81-167): cv::calcOpticalFlowPyrLK (:113, window
 * 21 x 21, 3 pyramid levels above the image, 30 iterations, epsilon 0.01), the inBorder cut (:5-11, :115-117), setMask (:36-69) and
 * cv::goodFeaturesToTrack (:149, quality 0.01, MIN_DIST, the mask).  Both images' pyramids stay on the device; per image only the image
 * and the points go up and the results come back.
 *
 * OpenCV is neither on the machines this was written on nor in the reference tree, so this is a RESTATEMENT WITH A WRITTEN CONTRACT, as
 * vilscan.h is for PCL, not a reproduction of OpenCV's bits.  It keeps OpenCV's structure -- fixed-point patch interpolation, integer
 * Scharr / Sobel derivatives, integer accumulations -- so that every sum of the hot loops is a sum of integers below 2^53, exact in any
 * order: the device equals tests/track_ref.py bit for bit with no summation order to agree on.
 *
 * STAYS ON THE HOST (out of scope here):
 *   - CLAHE (equalize: 1, :87-93): not here, but on the device all the same, in the row behind vilclahe.h: vclahe_push equalises the raw
 *     image straight into this tracker's next image and builds its pyramid; vtrack_push_image takes an image as it is.
 *   - rejectWithF (:169-202) and undistortedPoints (:258-306) with the PINHOLE camera model: not here, but on the device all the same,
 *     in the row of their own behind vilepi.h (vepi_reject, vepi_undistort).
 *   - ids, track_cnt, reduceVector and addPoints: the caller compacts its vectors on `status` and `kept` -- or leaves all of it on the
 *     device: vfeat_read_image (vilfeat.h) is readImage as one call over the kernels of this row, with the points resident.
 *   - the sort by track_cnt in setMask (:50-53): an unstable std::sort; tracks_xy arrives in the caller's priority order (vilfeat.h
 *     fixes it as the stable order).
 *   - the PUB_THIS_FRAME schedule: vtrack_detect is called when the reference would call setMask.
 *   - the fisheye mask (FISHEYE, :38-39): the mask of step 7 starts as all 255.
 *
 * ARITHMETIC CONTRACT.  f32 is unfused IEEE float32 in the order written; everything else is integer (>> is an arithmetic shift).
 * r101(i, n) is the reflect-101 index with period 2(n-1), valid for any i (0 when n = 1).  M(u, v) for a per-pixel map M and ANY integer
 * (u, v) means M[r101(v, H)][r101(u, W)]; I is an image level, Ix / Iy its derivative maps.
 *   1 pyramid     level l+1 has size ((W+1)/2, (H+1)/2): out(x, y) = (sum_ij k_i k_j I(2x+j-2, 2y+i-2) + 128) >> 8, k = [1 4 6 4 1].
 *   2 derivatives Ix(x, y) = 3 (I(x+1, y-1) - I(x-1, y-1)) + 10 (I(x+1, y) - I(x-1, y)) + 3 (I(x+1, y+1) - I(x-1, y+1)) at the pixels of
 *                 the level, Iy the transpose.  DEVIATION: a window sample outside the level reads the derivative MAP through r101 (the
 *                 derivative of the reflected pixel), where OpenCV pads the derivative image with zeros.
 *   3 per point   status = 1; levels l = max_level .. 0: prev = pt * 2^-l (f32); next = prev at l = max_level, else next = next * 2.
 *                 p = prev - 10, fp = floorf(p).  Bounds test B(f): -21 <= f.x < W_l and -21 <= f.y < H_l, compared as f32 (false for
 *                 NaN).  When B(fp) fails: code SKIP, at level 0 status = 0, next stays as it is, on to the next level.
 *   4 template    a = p.x - fp.x, b = p.y - fp.y (f32).  w00 = rint((1-a)*(1-b)*16384), w01 = rint(a*(1-b)*16384), w10 = rint((1-a)*b*16384),
 *                 w11 = 16384 - w00 - w01 - w10; rint is half-even; w01 weighs the pixel at x+1, w10 the one at y+1.  With ip = int(fp) and
 *                 S_M(x, y) = w00 M(ip.x+x, ip.y+y) + w01 M(ip.x+x+1, ip.y+y) + w10 M(ip.x+x, ip.y+y+1) + w11 M(ip.x+x+1, ip.y+y+1) over
 *                 the 21 x 21 window: Iw = (S_I + 256) >> 9, Dx = (S_Ix + 8192) >> 14, Dy = (S_Iy + 8192) >> 14.
 *                 A11 = f32(sum Dx^2) * 2^-20, A12 = f32(sum Dx Dy) * 2^-20, A22 = f32(sum Dy^2) * 2^-20: exact 64-bit sums, converted
 *                 once (round to nearest even).  D = A11*A22 - A12*A12; minEig = ((A22 + A11) - sqrtf((A11-A22)*(A11-A22) + (4*A12)*A12)) / 882.
 *                 When minEig < 1e-4f || D < FLT_EPSILON: code LOWEIG, at level 0 status = 0, on to the next level.  Otherwise D = 1 / D.
 *   5 iterations  next -= 10; at most 30 times: fn = floorf(next); when B(fn) fails: code OOB, at level 0 status = 0, the level ends.
 *                 Jw as Iw, on the other image at fn with the fractions of next; diff = Jw - Iw; b1 = f32(sum diff Dx) * 2^-20, b2 =
 *                 f32(sum diff Dy) * 2^-20; d = ((A12*b2 - A22*b1)*D, (A12*b1 - A11*b2)*D); next += d.  Code EPS when d.x*d.x + d.y*d.y
 *                 <= 1e-4f.  From the second iteration on, code OSC when |d.x + dprev.x| < 0.01f && |d.y + dprev.y| < 0.01f, then next -=
 *                 d * 0.5f.  Code CAP after the 30th iteration.  After the loop next += 10.  The iteration count of a level is the number
 *                 of steps d applied.
 *   6 border cut  r = rintf(next) of level 0; status &= 1 <= r.x < W-1 && 1 <= r.y < H-1, compared as f32.  DEVIATION: a non-finite
 *                 result gives status 0 (cvRound of NaN is undefined).  forw_xy is next whatever the status.
 *   7 setMask     track i's pixel is (rintf(x), rintf(y)).  It is kept iff the pixel is inside the image (compared as f32) and no EARLIER
 *                 KEPT track's pixel lies within dx^2 + dy^2 <= min_dist^2.  The mask is 0 within that disc of any kept track, 255
 *                 elsewhere.  DEVIATIONS: cv::circle's rasterisation is replaced by the exact disc; a pixel outside the image is dropped
 *                 where the reference reads the mask out of bounds.
 *   8 response    Sobel dx(x, y) = (I(x+1, y-1) + 2 I(x+1, y) + I(x+1, y+1)) - (the same at x-1), dy the transpose; Sxx, Sxy, Syy the 3 x 3
 *                 box sums of dx dx, dx dy, dy dy, with (dx dx)(u, v) read through r101 as a map.  s = 1.0f / 3060.0f, s2 = s * s;
 *                 a = f32(Sxx)*s2*0.5f, b = f32(Sxy)*s2, c = f32(Syy)*s2*0.5f; eig = (a + c) - sqrtf((a-c)*(a-c) + b*b).
 *   9 candidates  thr = max(eig over pixels with mask 255 and eig > 0; 0 without one) * quality.  A pixel with 1 <= x < W-1, 1 <= y < H-1
 *                 is a candidate when eig > thr, eig equals the 3 x 3 maximum (through r101) of the map thresholded at thr, and its mask
 *                 is 255.  Rank: eig descending, then pixel index y*W + x ascending (a restatement: OpenCV breaks ties by address).
 *  10 picks       in rank order a candidate is picked iff no earlier pick lies within dx^2 + dy^2 < min_dist^2; the first
 *                 max(0, max_cnt - n_kept) picks are returned as (float(x), float(y)).  The device decides the picks by a fixpoint over
 *                 the candidates (picked iff no PICKED candidate of higher rank is that close) and ranks only the survivors; the fixpoint
 *                 is unique, so neither the list nor its order depends on timing.
 * Plain C, POD only, host pointers.  Needs a HIP device; there is no CPU fallback. */
#ifndef VILTRACK_H
#define VILTRACK_H
#include <stdint.h>
#include "vilsolve.h"
#ifdef __cplusplus
extern "C" {
#endif

#define VTRACK_NUM_KERNELS 8         /* k_track_pyr, k_track_lk, k_track_mask, k_track_paint, k_track_eig, k_track_cand, k_track_round, k_track_pick */
#define VTRACK_MAX_LEVEL 3
#define VTRACK_MAX_POINTS_LIMIT 4096 /* setMask keeps its tracks in LDS */
#define VTRACK_MAX_MIN_DIST 1024
#define VTRACK_WIN 21
#define VTRACK_MAX_ITERS 30

/* termination code of a point at a level (step 5, and the two ways a level is left before it) */
enum { VTRACK_CODE_SKIP = 0, VTRACK_CODE_LOWEIG = 1, VTRACK_CODE_EPS = 2, VTRACK_CODE_OSC = 3, VTRACK_CODE_CAP = 4, VTRACK_CODE_OOB = 5 };
/* what vtrack_debug_read returns */
enum { VTRACK_DBG_CUR_LEVEL = 0, VTRACK_DBG_FORW_LEVEL = 1, VTRACK_DBG_LK_CODES = 2, VTRACK_DBG_LK_ITERS = 3, VTRACK_DBG_EIG = 4, VTRACK_DBG_MASK = 5,
       VTRACK_DBG_N_CANDIDATES = 6 };

typedef struct vtrack_ctx vtrack_ctx;

typedef struct vtrack_cfg {
    int32_t width, height;       /* 16 .. 16384 each */
    int32_t max_level;           /* 0 .. VTRACK_MAX_LEVEL; reference: 3 */
    int32_t max_points;          /* 1 .. VTRACK_MAX_POINTS_LIMIT: points of a vtrack_track, tracks of a vtrack_detect */
    int32_t max_candidates;      /* room for step 9's candidates (a noisy 640 x 480 image has about 18 k) */
} vtrack_cfg;

typedef struct vtrack_summary {
    int32_t n_points, n_tracked;            /* vtrack_track: points given, points with status 1 */
    int32_t n_tracks, n_kept;               /* vtrack_detect: tracks given, tracks setMask kept */
    int32_t n_candidates, n_picked, n_new;  /* step 9's candidates, step 10's picks before the max_cnt cut, corners returned */
    int32_t rounds;                         /* rounds of step 10's fixpoint, the four device-wide ones included (a measurement: it may differ between runs, the picks do not) */
} vtrack_summary;

/* All device and pinned memory is allocated here.  VIL_ERR_INVALID_ARGUMENT for a NULL pointer or a size outside the ranges above, then
 * VIL_ERR_DEVICE without a HIP device. */
int vtrack_create(int32_t device, const vtrack_cfg* cfg, vtrack_ctx** out);
void vtrack_destroy(vtrack_ctx* ctx);
/* gray: height rows of width bytes, row_stride bytes apart.  The image becomes forw and the previous forw becomes cur; on the first image
 * cur = forw (:97-100).  Builds forw's pyramid: one upload, max_level launches.  VIL_ERR_INVALID_ARGUMENT when row_stride < width; the
 * resident images stay as they were. */
int vtrack_push_image(vtrack_ctx* ctx, const uint8_t* gray, int32_t row_stride);
/* cur_xy: n points [x y] in cur.  forw_xy (2n floats) and status (n bytes) are written for every point: status is LK's status AND
 * inBorder(forw) (step 6).  One upload, one launch, one read-back.  VIL_ERR_INVALID_ARGUMENT when n > max_points or before the first
 * image; nothing is written then.  `out` may be NULL. */
int vtrack_track(vtrack_ctx* ctx, int32_t n, const float* cur_xy, float* forw_xy, uint8_t* status, vtrack_summary* out);
/* Steps 7-10 on forw.  tracks_xy: n_tracks points in priority order; kept: n_tracks bytes, setMask's decision; new_xy: room for max_cnt
 * points, *n_new of them written in pick order -- none when n_kept >= max_cnt (:140-152; the response, the mask and the candidates are
 * computed all the same, for vtrack_debug_read).  quality in (0, 1], min_dist in [0, VTRACK_MAX_MIN_DIST], max_cnt >= 0.  One upload,
 * two clears, nine launches
 * (k_track_round four times), one read-back.  VIL_ERR_INVALID_ARGUMENT for n_tracks > max_points, a bad parameter or no image;
 * VIL_ERR_UNSUPPORTED when the candidates exceed max_candidates (never truncated).  Neither writes any output. */
int vtrack_detect(vtrack_ctx* ctx, int32_t n_tracks, const float* tracks_xy, int32_t min_dist, int32_t max_cnt, float quality, uint8_t* kept, int32_t* n_new,
                  float* new_xy, vtrack_summary* out);
/* test hook.  what = VTRACK_DBG_CUR_LEVEL / _FORW_LEVEL: level `arg` of that image, W_l x H_l bytes.  _LK_CODES / _LK_ITERS: of the last
 * vtrack_track, n x (max_level + 1) bytes, byte [i][l] for point i at level l.  _EIG: step 8's map (W x H floats), _MASK: step 7's mask
 * (W x H bytes), _N_CANDIDATES: one int32, all of the last vtrack_detect.  VIL_ERR_INVALID_ARGUMENT when capacity_bytes is too small. */
int vtrack_debug_read(vtrack_ctx* ctx, int32_t what, int32_t arg, void* dst, int64_t capacity_bytes);
/* measurement hook, as vscan_profile_*: HIP events around the kernels; read returns the launch counts and total durations of the
 * VTRACK_NUM_KERNELS kernels in the order listed above and resets them */
int vtrack_profile_enable(vtrack_ctx* ctx, int32_t enable);
int vtrack_profile_read(vtrack_ctx* ctx, int64_t* launches8, double* total_ms8);

#ifdef __cplusplus
}
#endif
#endif
