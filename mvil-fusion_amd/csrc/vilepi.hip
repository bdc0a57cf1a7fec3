// vilepi.hip -- epipolar outlier rejection and undistortion of tracked points on gfx950 behind include/vilepi.h (feature_tracker_/src/
// feature_tracker.cpp: rejectWithF :169-202, undistortedPoints :258-306; the steps are numbered as in the header).
//
//   k_epi_lift     a thread per point of either image: steps 1-2, the float32 points of the virtual camera.
//   k_epi_hyp      a WAVE (= workgroup of 64) per hypothesis: steps 3-5.  Lane 0 draws the sample, lanes 0 / 1 normalise the two images, lanes
//                  0-7 write the eight rows, A^T A sits in LDS with one lane per entry summing in sample order.  The Jacobi is the serial
//                  chain of the launch: every rotation is two barriers, the angle computed by all lanes from the same three entries, lanes
//                  0-8 each rotating one row pair of A (and its mirror) and lanes 16-24 one row of V -- the elements of one rotation are
//                  independent, so the arithmetic per element is that of the serial loop.  The n points are scored 64 at a time; a ballot is
//                  the word of the hypothesis' row in the inlier table and its popcount goes to the count.  No floating-point sum depends on
//                  lane order (the margin is a minimum), no atomics.
//   k_epi_undist   a thread per point: step 8; the previous table's ids staged in LDS and searched by brute force for the first occurrence
//                  (setMask reorders by track_cnt, so ids are not sorted).
// The host replays step 6 over the counts of each batch and launches the next batch only while the loop has not ended.
// The double arithmetic of the contract is unfused and in source order:
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/vilepi.h"
#include "vil_host.hpp"
#include "vilepi_stage.hpp"

#define VE_MAX_DRAWS 65536                // step 3 gives up (no model) after this many draws: n = 8 needs 22 on average, the chance of 65536 is (7/8)^65000

namespace {

struct Cam { double iK11, iK13, iK22, iK23, k1, k2, p1, p2, focal, half_w, half_h; int no_distortion; };

// ---- step 1 ----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void distortion(const Cam& c, const double x, const double y, double& dx, double& dy) {
    const double mx2 = x * x, my2 = y * y, mxy = x * y;
    const double rho2 = mx2 + my2;
    const double rad = c.k1 * rho2 + c.k2 * rho2 * rho2;
    dx = x * rad + 2.0 * c.p1 * mxy + c.p2 * (rho2 + 2.0 * mx2);
    dy = y * rad + 2.0 * c.p2 * mxy + c.p1 * (rho2 + 2.0 * my2);
}
__device__ __forceinline__ void lift(const Cam& c, const float u, const float v, double& xu, double& yu) {
    const double xd = c.iK11 * (double)u + c.iK13, yd = c.iK22 * (double)v + c.iK23;
    xu = xd; yu = yd;
    if (c.no_distortion) return;
    double dx, dy;
    for (int i = 0; i < VEPI_LIFT_STEPS; ++i) {
        distortion(c, xu, yu, dx, dy);
        xu = xd - dx; yu = yd - dy;
    }
}

// step 2: threads 0 .. n_max - 1 take the points of cur, the next n_max those of forw.  n_dev: NULL, or where the count is read from (<= n_max)
__global__ __launch_bounds__(256) void k_epi_lift(const Cam cam, int n_max, const int* __restrict__ n_dev, const float2* __restrict__ cur, const float2* __restrict__ forw,
                                                  float2* __restrict__ p1, float2* __restrict__ p2) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= 2 * n_max) return;
    const int second = t >= n_max ? 1 : 0, i = t - second * n_max;
    if (i >= (n_dev ? min(n_max, *n_dev) : n_max)) return;
    const float2 p = second ? forw[i] : cur[i];
    double x, y;
    lift(cam, p.x, p.y, x, y);
    const float2 o = make_float2((float)(cam.focal * x + cam.half_w), (float)(cam.focal * y + cam.half_h));
    if (second) p2[i] = o; else p1[i] = o;
}

// ---- steps 3-5 -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long mix64(unsigned long long x) {
    unsigned long long z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// cyclic Jacobi of the symmetric N x N matrix A in LDS, V = I on entry; one wave, every lane calls it
template <int N>
__device__ void jacobi(double* A, double* V, const int lane) {
#pragma unroll 1
    for (int sweep = 0; sweep < VEPI_JACOBI_SWEEPS; ++sweep)
#pragma unroll 1
        for (int p = 0; p < N - 1; ++p)
#pragma unroll 1
            for (int q = p + 1; q < N; ++q) {
                const double apq = A[p * N + q], app = A[p * N + p], aqq = A[q * N + q];            // the same three entries in every lane
                __syncthreads();                                                                    // read before lanes p and q overwrite them
                if (apq != 0.0) {
                    const double theta = (aqq - app) / (2.0 * apq);
                    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                    const double c = 1.0 / sqrt(t * t + 1.0);
                    const double s = t * c;
                    if (lane < N) {
                        const int k = lane;
                        if (k == p) { A[p * N + p] = app - t * apq; A[p * N + q] = 0.0; }
                        else if (k == q) { A[q * N + q] = aqq + t * apq; A[q * N + p] = 0.0; }
                        else {                                                                      // row k's pair and its mirror: no other lane touches them
                            const double akp = A[k * N + p], akq = A[k * N + q];
                            const double np = c * akp - s * akq, nq = s * akp + c * akq;
                            A[k * N + p] = np; A[p * N + k] = np; A[k * N + q] = nq; A[q * N + k] = nq;
                        }
                    } else if (lane >= 16 && lane < 16 + N) {
                        const int k = lane - 16;
                        const double vkp = V[k * N + p], vkq = V[k * N + q];
                        V[k * N + p] = c * vkp - s * vkq; V[k * N + q] = s * vkp + c * vkq;
                    }
                }
                __syncthreads();
            }
}
// index of the smallest diagonal entry, the lowest among equal ones
template <int N>
__device__ __forceinline__ int smallest(const double* A) {
    int best = 0;
    double val = A[0];
    for (int k = 1; k < N; ++k) if (A[k * N + k] < val) { val = A[k * N + k]; best = k; }
    return best;
}

// n_dev: NULL, or where the count is read from; below the minimal sample there is nothing to do (the host does not launch for such an n)
__global__ __launch_bounds__(64) void k_epi_hyp(int n, const int* __restrict__ n_dev, int h0, unsigned long long seed, double thr2, const float2* __restrict__ p1,
                                                const float2* __restrict__ p2, int* __restrict__ samples, int* __restrict__ counts, double* __restrict__ margins,
                                                double* __restrict__ Fout, unsigned long long* __restrict__ bits, int stride) {
    __shared__ double s_A[81], s_V[81], s_R[72], s_M[9], s_W[9], s_Fn[9], s_nrm[6];
    __shared__ int s_idx[VEPI_SAMPLE], s_ok[3];
    if (n_dev) {
        n = min(n, *n_dev);
        if (n < VEPI_SAMPLE) return;                                                                // the whole workgroup, before any barrier
    }
    const int lane = threadIdx.x, h = h0 + blockIdx.x;                                              // h < max_iters: the host clips the grid
    if (lane == 0) {                                                                                // step 3
        const unsigned long long base = seed ^ ((unsigned long long)h * 0xD1342543DE82EF95ull);
        int got = 0, k = 0;
        for (; got < VEPI_SAMPLE && k < VE_MAX_DRAWS; ++k) {
            const unsigned long long r = mix64(base + (unsigned long long)k);
            const int i = (int)(((r >> 32) * (unsigned long long)n) >> 32);                        // < n
            bool dup = false;
            for (int j = 0; j < got; ++j) dup |= s_idx[j] == i;
            if (!dup) s_idx[got++] = i;
        }
        s_ok[2] = got == VEPI_SAMPLE;
        for (int j = got; j < VEPI_SAMPLE; ++j) s_idx[j] = 0;
        for (int j = 0; j < VEPI_SAMPLE; ++j) samples[h * VEPI_SAMPLE + j] = s_idx[j];
    }
    __syncthreads();
    if (lane < 2) {                                                                                 // step 4: the normalisation of image `lane`
        const float2* pts = lane ? p2 : p1;
        double sx = 0.0, sy = 0.0;
        for (int r = 0; r < VEPI_SAMPLE; ++r) {
            const float2 p = pts[s_idx[r]];
            if (r == 0) { sx = (double)p.x; sy = (double)p.y; } else { sx = sx + (double)p.x; sy = sy + (double)p.y; }
        }
        const double cx = sx / 8.0, cy = sy / 8.0;
        double d = 0.0;
        for (int r = 0; r < VEPI_SAMPLE; ++r) {
            const float2 p = pts[s_idx[r]];
            const double dx = (double)p.x - cx, dy = (double)p.y - cy;
            const double e = sqrt(dx * dx + dy * dy);
            d = r == 0 ? e : d + e;
        }
        const double mean = d / 8.0;
        s_ok[lane] = mean > 0.0;
        s_nrm[3 * lane] = cx; s_nrm[3 * lane + 1] = cy; s_nrm[3 * lane + 2] = sqrt(2.0) / mean;
    }
    __syncthreads();
    const double c1x = s_nrm[0], c1y = s_nrm[1], s1 = s_nrm[2], c2x = s_nrm[3], c2y = s_nrm[4], s2 = s_nrm[5];
    if (lane < VEPI_SAMPLE) {
        const float2 a = p1[s_idx[lane]], b = p2[s_idx[lane]];
        const double u1 = ((double)a.x - c1x) * s1, v1 = ((double)a.y - c1y) * s1, u2 = ((double)b.x - c2x) * s2, v2 = ((double)b.y - c2y) * s2;
        double* R = s_R + 9 * lane;
        R[0] = u2 * u1; R[1] = u2 * v1; R[2] = u2; R[3] = v2 * u1; R[4] = v2 * v1; R[5] = v2; R[6] = u1; R[7] = v1; R[8] = 1.0;
    }
    __syncthreads();
    for (int e = lane; e < 81; e += 64) {
        const int i = e / 9, j = e - 9 * i;
        double acc = s_R[i] * s_R[j];
        for (int r = 1; r < VEPI_SAMPLE; ++r) acc = acc + s_R[9 * r + i] * s_R[9 * r + j];
        s_A[e] = acc; s_V[e] = i == j ? 1.0 : 0.0;
    }
    __syncthreads();
    jacobi<9>(s_A, s_V, lane);
    const int col = smallest<9>(s_A);
    if (lane < 9) s_Fn[lane] = s_V[lane * 9 + col];
    __syncthreads();
    if (lane < 9) {
        const int i = lane / 3, j = lane - 3 * i;
        s_M[lane] = (s_Fn[i] * s_Fn[j] + s_Fn[3 + i] * s_Fn[3 + j]) + s_Fn[6 + i] * s_Fn[6 + j];
        s_W[lane] = i == j ? 1.0 : 0.0;
    }
    __syncthreads();
    jacobi<3>(s_M, s_W, lane);
    const int c3 = smallest<3>(s_M);
    const double v0 = s_W[c3], v1 = s_W[3 + c3], v2 = s_W[6 + c3];
    const double t1x = -(s1 * c1x), t1y = -(s1 * c1y), t2x = -(s2 * c2x), t2y = -(s2 * c2y);
    double G[3][3], F[3][3];                                                                        // every lane: the 3 x 3 tail is cheaper than a broadcast
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double a = s_Fn[3 * i], b = s_Fn[3 * i + 1], c = s_Fn[3 * i + 2];
        const double w = (a * v0 + b * v1) + c * v2;
        const double f0 = a - w * v0, f1 = b - w * v1, f2 = c - w * v2;
        G[i][0] = f0 * s1; G[i][1] = f1 * s1; G[i][2] = (f0 * t1x + f1 * t1y) + f2;
    }
    bool ok = s_ok[0] && s_ok[1] && s_ok[2];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        F[0][j] = G[0][j] * s2; F[1][j] = G[1][j] * s2; F[2][j] = (G[0][j] * t2x + G[1][j] * t2y) + G[2][j];
        ok = ok && isfinite(F[0][j]) && isfinite(F[1][j]) && isfinite(F[2][j]);
    }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) Fout[h * 9 + 3 * i + j] = ok ? F[i][j] : 0.0;               // constant indices: F stays in registers
    }
    int cnt = 0;                                                                                    // step 5
    double margin = INFINITY;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        bool inl = false;
        if (ok && i < n) {
            const float2 a = p1[i], b = p2[i];
            const double x1 = (double)a.x, y1 = (double)a.y, x2 = (double)b.x, y2 = (double)b.y;
            double la = (F[0][0] * x1 + F[0][1] * y1) + F[0][2], lb = (F[1][0] * x1 + F[1][1] * y1) + F[1][2], lc = (F[2][0] * x1 + F[2][1] * y1) + F[2][2];
            double d = (x2 * la + y2 * lb) + lc;
            const double e2 = (d * d) * (1.0 / (la * la + lb * lb));
            la = (F[0][0] * x2 + F[1][0] * y2) + F[2][0]; lb = (F[0][1] * x2 + F[1][1] * y2) + F[2][1]; lc = (F[0][2] * x2 + F[1][2] * y2) + F[2][2];
            d = (x1 * la + y1 * lb) + lc;
            const double e1 = (d * d) * (1.0 / (la * la + lb * lb));
            inl = e1 <= thr2 && e2 <= thr2;                                                        // false for NaN
            const double m = fabs((e1 > e2 ? e1 : e2) / thr2 - 1.0);
            if (m < margin) margin = m;                                                             // a NaN is ignored
        }
        const unsigned long long word = __ballot(inl);                                              // all 64 lanes get here
        if (lane == 0) bits[(size_t)h * stride + (base >> 6)] = word;                               // base / 64 < ceil(n / 64) <= stride
        cnt += __popcll(word);
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) margin = fmin(margin, __shfl_xor(margin, o));                      // a minimum: exact in any order
    if (lane == 0) { counts[h] = cnt; margins[h] = margin; }
}

// ---- step 8 ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_epi_undist(const Cam cam, int n, const int* __restrict__ n_dev, const float2* __restrict__ xy, const int* __restrict__ ids, double dt,
                                                    int n_prev, const int* __restrict__ prev_ids, const float2* __restrict__ prev_un, int* __restrict__ new_ids,
                                                    float2* __restrict__ new_un, float2* __restrict__ un_out, float2* __restrict__ vel_out) {
    __shared__ int s_ids[VEPI_MAX_POINTS_LIMIT];
    for (int j = threadIdx.x; j < n_prev; j += 256) s_ids[j] = prev_ids[j];                         // n_prev <= max_points <= VEPI_MAX_POINTS_LIMIT
    __syncthreads();
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (n_dev) n = min(n, *n_dev);
    if (t >= n) return;
    const float2 p = xy[t];
    double x, y;
    lift(cam, p.x, p.y, x, y);
    const float2 un = make_float2((float)x, (float)y);
    const int id = ids[t];
    float2 vel = make_float2(0.f, 0.f);
    if (id != -1) {
        int hit = -1;
        for (int j = 0; j < n_prev; ++j) if (s_ids[j] == id) { hit = j; break; }                   // the first occurrence
        if (hit >= 0) {
            const float2 pv = prev_un[hit];
            vel = make_float2((float)(((double)un.x - (double)pv.x) / dt), (float)(((double)un.y - (double)pv.y) / dt));
        }
    }
    un_out[t] = un; vel_out[t] = vel; new_ids[t] = id; new_un[t] = un;
}

// step 6's N
int update_iters(const double confidence, const double ratio, const int max_iters) {
    double den = 1.0 - pow(1.0 - ratio, (double)VEPI_SAMPLE);
    if (den < DBL_MIN) return 0;
    const double num = log(1.0 - confidence);
    den = log(den);
    return den >= 0.0 || -num >= max_iters * -den ? max_iters : (int)rint(num / den);
}

}  // namespace

struct vepi_ctx : vilhost::Device {          // d_mem: cur, forw | p1 | p2 | samples | counts | margins | F | bits | undistort: xy, ids | out un, vel | table 0 | table 1
    vepi_cfg cfg = {};
    Cam cam = {};
    int words = 0;                           // 64-bit words of a row of the inlier table
    char* h_in = nullptr; char* h_out = nullptr; char* h_res = nullptr;     // h_res (VEPI_READBACK_PINNED): counts | bits, written by k_epi_hyp
    int* k_counts = nullptr; unsigned long long* k_bits = nullptr;          // where k_epi_hyp writes them: the arena or h_res
    size_t o_in = 0, o_p1 = 0, o_p2 = 0, o_samples = 0, o_counts = 0, o_margins = 0, o_F = 0, o_bits = 0, o_uin = 0, o_uout = 0, o_tab[2] = {};
    int tab = 0, n_tab = 0;                  // the slot that holds the previous table and its length
    int dbg_n = 0, dbg_eval = 0, dbg_best = -1;
    vilhost::EventLog<VEPI_NUM_KERNELS> prof;
};

// ---- the stages (vilepi_stage.hpp): the launches, on the caller's pointers and stream ---------------------------------------------
vilepi_stage::Buffers vilepi_stage::buffers(const vepi_ctx* c) {
    char* d = c->d_mem;
    return {(float2*)(d + c->o_p1), (float2*)(d + c->o_p2), (int*)(d + c->o_samples), (int*)(d + c->o_counts), (double*)(d + c->o_margins), (double*)(d + c->o_F),
            (unsigned long long*)(d + c->o_bits), c->words};
}

void vilepi_stage::lift(const vepi_ctx* c, hipStream_t stream, const int n_max, const int* d_n, const float2* cur, const float2* forw, float2* p1, float2* p2) {
    hipLaunchKernelGGL(k_epi_lift, dim3((2 * n_max + 255) / 256), dim3(256), 0, stream, c->cam, n_max, d_n, cur, forw, p1, p2);
}

void vilepi_stage::hypotheses(const vepi_ctx* c, hipStream_t stream, const int n_max, const int* d_n, const int h0, const int B, const uint64_t seed, const double thr2,
                              const Buffers& b, int* counts, unsigned long long* bits) {
    hipLaunchKernelGGL(k_epi_hyp, dim3(B), dim3(64), 0, stream, n_max, d_n, h0, (unsigned long long)seed, thr2, (const float2*)b.p1, (const float2*)b.p2, b.samples, counts,
                       b.margins, b.F, bits, b.words);
}

void vilepi_stage::undistort(const vepi_ctx* c, hipStream_t stream, const int n_max, const int* d_n, const float2* xy, const int* ids, const double dt, const int n_prev,
                             const int* prev_ids, const float2* prev_un, int* new_ids, float2* new_un, float2* un_out, float2* vel_out) {
    hipLaunchKernelGGL(k_epi_undist, dim3((n_max + 255) / 256), dim3(256), 0, stream, c->cam, n_max, d_n, xy, ids, dt, n_prev, prev_ids, prev_un, new_ids, new_un, un_out, vel_out);
}

int vilepi_stage::update_iters(const double confidence, const double outlier_ratio, const int max_iters) { return ::update_iters(confidence, outlier_ratio, max_iters); }

extern "C" {

int vepi_create(int32_t device, const vepi_cfg* cfg, vepi_ctx** out) {
    if (!out || !cfg || !std::isfinite(cfg->fx) || !std::isfinite(cfg->fy) || cfg->fx == 0.0 || cfg->fy == 0.0 || !std::isfinite(cfg->cx) || !std::isfinite(cfg->cy) ||
        !std::isfinite(cfg->k1) || !std::isfinite(cfg->k2) || !std::isfinite(cfg->p1) || !std::isfinite(cfg->p2) || !std::isfinite(cfg->focal) || cfg->width < 1 ||
        cfg->width > 65536 || cfg->height < 1 || cfg->height > 65536 || cfg->model < VEPI_MODEL_PINHOLE || cfg->model > VEPI_MODEL_SCARAMUZZA ||
        cfg->max_points < VEPI_MIN_POINTS_LIMIT || cfg->max_points > VEPI_MAX_POINTS_LIMIT || cfg->max_iters < 1 || cfg->max_iters > VEPI_MAX_ITERS_LIMIT || cfg->batch < 0 ||
        cfg->batch > cfg->max_iters || (cfg->readback != VEPI_READBACK_COPY && cfg->readback != VEPI_READBACK_PINNED))
        return VIL_ERR_INVALID_ARGUMENT;
    if (cfg->model != VEPI_MODEL_PINHOLE) return VIL_ERR_UNSUPPORTED;
    vepi_ctx* c = new vepi_ctx();
    c->cfg = *cfg;
    if (!c->cfg.batch) c->cfg.batch = cfg->max_iters;
    Cam& m = c->cam;
    m.iK11 = 1.0 / cfg->fx; m.iK13 = -cfg->cx / cfg->fx; m.iK22 = 1.0 / cfg->fy; m.iK23 = -cfg->cy / cfg->fy;
    m.k1 = cfg->k1; m.k2 = cfg->k2; m.p1 = cfg->p1; m.p2 = cfg->p2;
    m.focal = cfg->focal; m.half_w = cfg->width / 2.0; m.half_h = cfg->height / 2.0;
    m.no_distortion = cfg->k1 == 0.0 && cfg->k2 == 0.0 && cfg->p1 == 0.0 && cfg->p2 == 0.0;
    const size_t P = (size_t)cfg->max_points, MI = (size_t)cfg->max_iters;
    c->words = (int)((P + 63) / 64);
    vilhost::Arena a;
    c->o_in = a.take(16 * P);
    c->o_p1 = a.take(8 * P); c->o_p2 = a.take(8 * P);
    c->o_samples = a.take(4 * VEPI_SAMPLE * MI); c->o_counts = a.take(4 * MI); c->o_margins = a.take(8 * MI); c->o_F = a.take(72 * MI);
    c->o_bits = a.take(8 * (size_t)c->words * MI);
    c->o_uin = a.take(12 * P); c->o_uout = a.take(16 * P);
    c->o_tab[0] = a.take(12 * P); c->o_tab[1] = a.take(12 * P);          // ids, then un
    hipError_t err = c->open(device, a.bytes);
    if (err == hipSuccess) err = c->pin(&c->h_in, 16 * P);
    if (err == hipSuccess) err = c->pin(&c->h_out, std::max(16 * P, std::max(4 * MI, 8 * (size_t)c->words)));
    if (err == hipSuccess) {
        c->k_counts = (int*)(c->d_mem + c->o_counts); c->k_bits = (unsigned long long*)(c->d_mem + c->o_bits);
        if (cfg->readback == VEPI_READBACK_PINNED) {
            const size_t cb = vilhost::up16(4 * MI);
            err = c->pin(&c->h_res, cb + 8 * (size_t)c->words * MI);
            void* dev = nullptr;
            if (err == hipSuccess) err = hipHostGetDevicePointer(&dev, c->h_res, 0);
            if (err == hipSuccess) { c->k_counts = (int*)dev; c->k_bits = (unsigned long long*)((char*)dev + cb); }
        }
    }
    if (err == hipSuccess) err = hipMemsetAsync(c->d_mem, 0, a.bytes, c->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(c->stream);
    if (err != hipSuccess) { vepi_destroy(c); VILCHK(err); }
    *out = c;
    return VIL_OK;
}

void vepi_destroy(vepi_ctx* c) {
    if (!c) return;
    c->close(c->prof);
    delete c;
}

int vepi_profile_enable(vepi_ctx* c, int32_t enable) {
    if (!c) return VIL_ERR_INVALID_ARGUMENT;
    c->prof.on = enable != 0;
    return VIL_OK;
}
int vepi_profile_read(vepi_ctx* c, int64_t* launches3, double* total_ms3) {
    if (!c || !launches3 || !total_ms3) return VIL_ERR_INVALID_ARGUMENT;
    c->prof.read(launches3, total_ms3);
    return VIL_OK;
}

int vepi_reject(vepi_ctx* c, int32_t n, const float* cur_xy, const float* forw_xy, double thr, double confidence, uint64_t seed, uint8_t* status, vepi_summary* out) {
    if (!c || n < 0 || n > c->cfg.max_points || (n && (!cur_xy || !forw_xy || !status)) || !(thr > 0.0) || !std::isfinite(thr) || !(confidence > 0.0 && confidence < 1.0))
        return VIL_ERR_INVALID_ARGUMENT;
    vepi_summary s = {};
    s.n_points = n; s.n_inliers = n; s.best_hypothesis = -1;
    if (n < VEPI_SAMPLE) {                                                                          // :171
        if (n) memset(status, 1, (size_t)n);
        if (out) *out = s;
        return VIL_OK;
    }
    VILCHK(hipSetDevice(c->device));
    char* d = c->d_mem;
    const bool pinned = c->cfg.readback == VEPI_READBACK_PINNED;
    const int max_iters = c->cfg.max_iters, words_n = (n + 63) / 64;
    memcpy(c->h_in, cur_xy, 8 * (size_t)n); memcpy(c->h_in + 8 * (size_t)n, forw_xy, 8 * (size_t)n);
    VILCHK(hipMemcpyAsync(d + c->o_in, c->h_in, 16 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    VILCHK(c->prof.mark(0, 1, c->stream));
    const vilepi_stage::Buffers buf = vilepi_stage::buffers(c);
    vilepi_stage::lift(c, c->stream, n, nullptr, (const float2*)(d + c->o_in), (const float2*)(d + c->o_in) + n, buf.p1, buf.p2);
    c->dbg_n = n; c->dbg_eval = 0; c->dbg_best = -1;
    int niters = max_iters, h = 0, best = 0, best_h = -1, h0 = 0;                                   // step 6
    const int* cnt = pinned ? (const int*)c->h_res : (const int*)c->h_out;                          // counts of hypotheses h0 ..: at cnt[pinned ? h : h - h0]
    while (h < niters) {
        const int B = std::min(c->cfg.batch, niters - h0);                                          // h == h0 here; h0 + B <= niters <= max_iters
        VILCHK(c->prof.mark(1, 1, c->stream));
        vilepi_stage::hypotheses(c, c->stream, n, nullptr, h0, B, seed, thr * thr, buf, c->k_counts, c->k_bits);
        VILCHK(c->prof.mark(-1, 0, c->stream));
        if (!pinned) VILCHK(hipMemcpyAsync(c->h_out, d + c->o_counts + 4 * (size_t)h0, 4 * (size_t)B, hipMemcpyDeviceToHost, c->stream));
        VILCHK(hipStreamSynchronize(c->stream));
        VILCHK(hipGetLastError());
        s.launches++; c->dbg_eval = h0 + B;
        for (; h < h0 + B && h < niters; ++h) {
            const int count = cnt[pinned ? h : h - h0];
            if (count > std::max(best, VEPI_SAMPLE - 1)) {
                best = count; best_h = h;
                niters = std::min(niters, update_iters(confidence, (double)(n - count) / (double)n, max_iters));
            }
        }
        h0 += B;
    }
    c->prof.collect();
    c->dbg_best = best_h;
    s.consumed = h; s.evaluated = c->dbg_eval;
    if (best_h < 0) {                                                                               // step 7
        memset(status, 1, (size_t)n);
        if (out) *out = s;
        return VIL_OK;
    }
    const unsigned long long* row = pinned ? (const unsigned long long*)(c->h_res + vilhost::up16(4 * (size_t)max_iters)) + (size_t)best_h * c->words : (const unsigned long long*)c->h_out;
    if (!pinned) {
        VILCHK(hipMemcpyAsync(c->h_out, d + c->o_bits + 8 * (size_t)best_h * c->words, 8 * (size_t)words_n, hipMemcpyDeviceToHost, c->stream));
        VILCHK(hipStreamSynchronize(c->stream));
    }
    for (int i = 0; i < n; ++i) status[i] = (uint8_t)((row[i >> 6] >> (i & 63)) & 1);
    s.found = 1; s.best_hypothesis = best_h; s.n_inliers = best;
    if (out) *out = s;
    return VIL_OK;
}

int vepi_undistort(vepi_ctx* c, int32_t n, const float* xy, const int32_t* ids, double dt, float* un_xy, float* vel_xy) {
    if (!c || n < 0 || n > c->cfg.max_points || (n && (!xy || !ids || !un_xy || !vel_xy))) return VIL_ERR_INVALID_ARGUMENT;
    if (n) {
        VILCHK(hipSetDevice(c->device));
        char* d = c->d_mem;
        const size_t P = (size_t)c->cfg.max_points;
        const int nt = 1 - c->tab;
        memcpy(c->h_in, xy, 8 * (size_t)n); memcpy(c->h_in + 8 * (size_t)n, ids, 4 * (size_t)n);
        VILCHK(hipMemcpyAsync(d + c->o_uin, c->h_in, 12 * (size_t)n, hipMemcpyHostToDevice, c->stream));
        VILCHK(c->prof.mark(2, 1, c->stream));
        vilepi_stage::undistort(c, c->stream, n, nullptr, (const float2*)(d + c->o_uin), (const int*)(d + c->o_uin + 8 * (size_t)n), dt, c->n_tab,
                                (const int*)(d + c->o_tab[c->tab]), (const float2*)(d + c->o_tab[c->tab] + 4 * P), (int*)(d + c->o_tab[nt]), (float2*)(d + c->o_tab[nt] + 4 * P),
                                (float2*)(d + c->o_uout), (float2*)(d + c->o_uout + 8 * (size_t)n));
        VILCHK(c->prof.mark(-1, 0, c->stream));
        VILCHK(hipMemcpyAsync(c->h_out, d + c->o_uout, 16 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
        VILCHK(hipStreamSynchronize(c->stream));
        VILCHK(hipGetLastError());
        c->prof.collect();
        memcpy(un_xy, c->h_out, 8 * (size_t)n); memcpy(vel_xy, c->h_out + 8 * (size_t)n, 8 * (size_t)n);
        c->tab = nt;
    }
    c->n_tab = n;
    return VIL_OK;
}

int vepi_reset(vepi_ctx* c) {
    if (!c) return VIL_ERR_INVALID_ARGUMENT;
    c->n_tab = 0;
    return VIL_OK;
}

int vepi_debug_read(vepi_ctx* c, int32_t what, void* dst, int64_t capacity_bytes) {
    if (!c || !dst || !c->dbg_n) return VIL_ERR_INVALID_ARGUMENT;
    const size_t n = (size_t)c->dbg_n, ev = (size_t)c->dbg_eval;
    size_t off = 0, bytes = 0;
    switch (what) {
    case VEPI_DBG_CUR_PTS: off = c->o_p1; bytes = 8 * n; break;
    case VEPI_DBG_FORW_PTS: off = c->o_p2; bytes = 8 * n; break;
    case VEPI_DBG_SAMPLES: off = c->o_samples; bytes = 4 * VEPI_SAMPLE * ev; break;
    case VEPI_DBG_COUNTS: off = c->o_counts; bytes = 4 * ev; break;
    case VEPI_DBG_MARGINS: off = c->o_margins; bytes = 8 * ev; break;
    case VEPI_DBG_F:
        if (c->dbg_best < 0) return VIL_ERR_INVALID_ARGUMENT;
        off = c->o_F + 72 * (size_t)c->dbg_best; bytes = 72; break;
    default: return VIL_ERR_INVALID_ARGUMENT;
    }
    if (capacity_bytes < (int64_t)bytes) return VIL_ERR_INVALID_ARGUMENT;
    if (what == VEPI_DBG_COUNTS && c->cfg.readback == VEPI_READBACK_PINNED) { memcpy(dst, c->h_res, bytes); return VIL_OK; }
    VILCHK(hipSetDevice(c->device));
    VILCHK(hipMemcpyAsync(dst, c->d_mem + off, bytes, hipMemcpyDeviceToHost, c->stream));
    VILCHK(hipStreamSynchronize(c->stream));
    return VIL_OK;
}

}  // extern "C"
