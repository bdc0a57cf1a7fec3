// viltrack.hip -- the KLT visual front end on gfx950 behind include/viltrack.h (feature_tracker_/src/feature_tracker.cpp: readImage
// :81-167; the steps are numbered as in the header).
//
// Both images' pyramids are resident; vtrack_push_image flips which slot is cur and which is forw.  Every entry point is one submission on
// the context's stream with one read-back.  vtrack_push_image is two stages, the upload into level 0 of the next slot and everything after
// it (viltrack_stage.hpp): vilclahe.hip produces level 0 on the device and shares the second.
//   k_track_pyr    a thread per pixel of level l+1: step 1, 25 bytes through r101.  One launch per level.
//   k_track_lk     a WAVE (= workgroup of 64) per point, the whole level loop in one launch: steps 3-6.  The 22 x 22 samples a window needs
//                  (image and, for the template, the Scharr derivatives computed on the fly from the image, step 2) are staged in LDS; a
//                  lane owns 7 of the 441 window positions and keeps their Iw / Dx / Dy in registers across the iterations.  Every sum is a
//                  64-bit integer sum reduced with shuffles -- exact, so its order does not matter -- and converted to f32 once.  All
//                  branches are wave-uniform: they depend on the point and on reduced sums only.
//   k_track_mask   ONE workgroup: step 7 as a fixpoint in LDS (a track is kept once every earlier close track is dropped, dropped once an
//                  earlier close track is kept).  k_track_paint: a workgroup per kept track clears its disc in the mask.
//   k_track_eig    a 16 x 16 tile per workgroup: Sobel products of the 18 x 18 pixels around it in LDS, box sums, step 8; the maximum of
//                  step 9 is an integer atomicMax on the bits of the positive floats, once per wave.
//   k_track_cand   a thread per pixel: step 9's candidates into a per-pixel map of their eig bits, a bitmap (a wave's ballot is the word of
//                  its 64 pixels) and an unordered list.
//   k_track_round  step 10's fixpoint, one round device-wide: a wave per undecided candidate, a lane per row of the disc around it -- the
//                  row's chord is a run of bits in the bitmap, so only candidates are visited.  VT_ROUNDS launches, then
//   k_track_pick   ONE workgroup runs the rounds that are left (usually none) until no candidate is undecided, ranks the picks among
//                  themselves by counting and writes the first `need` in rank order.
// A decision of either fixpoint is final and reads only final decisions, so updating in place cannot change the result, only the number
// of rounds; both loops are capped by their worst case (one decision per round) and report a cap that was hit as a device error.
// The float arithmetic of the contract is unfused and in source order (numpy does not contract a * b + c; hipcc would):
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/viltrack.h"
#include "vil_host.hpp"
#include "viltrack_stage.hpp"

#define VT_PATCH 22                       // VTRACK_WIN + 1 samples per side
#define VT_PATCH2 (VT_PATCH * VT_PATCH)
#define VT_WIN2 (VTRACK_WIN * VTRACK_WIN)
#define VT_PER_LANE 7                     // ceil(441 / 64)
#define VT_ONE_WG 1024
#define VT_ROUNDS 4                       // rounds of step 10's fixpoint that run device-wide before the single workgroup finishes it

using namespace viltrack_stage;                           // the counters of one detection, H_*

namespace {

__device__ __forceinline__ int r101(int i, const int n) {
    if ((unsigned)i < (unsigned)n) return i;
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    i %= p;
    if (i < 0) i += p;
    return i >= n ? p - i : i;                                                                      // in [0, n)
}

__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// ---- step 1 ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_track_pyr(const uint8_t* __restrict__ src, int W, int H, uint8_t* __restrict__ dst, int W2, int H2) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= W2 * H2) return;
    const int y = t / W2, x = t - y * W2;
    int xs[5], acc = 0;
#pragma unroll
    for (int j = 0; j < 5; ++j) xs[j] = r101(2 * x + j - 2, W);
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const uint8_t* row = src + (size_t)r101(2 * y + i - 2, H) * W;
        const int r = ((int)row[xs[0]] + 4 * (int)row[xs[1]]) + (6 * (int)row[xs[2]] + 4 * (int)row[xs[3]]) + (int)row[xs[4]];
        acc += (i == 0 || i == 4 ? 1 : (i == 2 ? 6 : 4)) * r;
    }
    dst[t] = (uint8_t)((acc + 128) >> 8);
}

// ---- steps 3-6 -------------------------------------------------------------------------------------------------------------------
struct Weights { int w00, w01, w10, w11; };
__device__ __forceinline__ Weights weights(const float a, const float b) {
    Weights w;
    w.w00 = (int)rintf(((1.0f - a) * (1.0f - b)) * 16384.0f);
    w.w01 = (int)rintf((a * (1.0f - b)) * 16384.0f);
    w.w10 = (int)rintf(((1.0f - a) * b) * 16384.0f);
    w.w11 = 16384 - w.w00 - w.w01 - w.w10;
    return w;
}
__device__ __forceinline__ bool lk_inside(const float fx, const float fy, const int W, const int H) {
    return fx >= -21.0f && fx < (float)W && fy >= -21.0f && fy < (float)H;                          // false for NaN
}
// the 22 x 22 samples at pixels (ix .. ix+21, iy .. iy+21) through r101; every index read lies inside the level
template <bool DERIV>
__device__ __forceinline__ void lk_stage(const uint8_t* __restrict__ img, const int W, const int H, const int ix, const int iy, const int lane, short* s_i, short* s_ix,
                                         short* s_iy) {
    for (int k = lane; k < VT_PATCH2; k += 64) {
        const int y = k / VT_PATCH, x = k - y * VT_PATCH;
        const int u = r101(ix + x, W), v = r101(iy + y, H);
        const uint8_t* r0 = img + (size_t)v * W;
        s_i[k] = (short)r0[u];
        if (DERIV) {
            const int um = r101(u - 1, W), up = r101(u + 1, W);
            const uint8_t* rm = img + (size_t)r101(v - 1, H) * W; const uint8_t* rp = img + (size_t)r101(v + 1, H) * W;
            const int a = rm[um], b = rm[u], c = rm[up], d = r0[um], e = r0[up], f = rp[um], g = rp[u], h = rp[up];
            s_ix[k] = (short)(3 * (c - a) + 10 * (e - d) + 3 * (h - f));
            s_iy[k] = (short)(3 * (f - a) + 10 * (g - b) + 3 * (h - c));
        }
    }
}
__device__ __forceinline__ int lk_interp(const short* s, const int q, const Weights w, const int rnd, const int sh) {
    return (w.w00 * (int)s[q] + w.w01 * (int)s[q + 1] + w.w10 * (int)s[q + VT_PATCH] + w.w11 * (int)s[q + VT_PATCH + 1] + rnd) >> sh;
}

// n_dev: NULL, or where the count is read from (<= n, the size of the grid)
__global__ __launch_bounds__(64) void k_track_lk(int n, const int* __restrict__ n_dev, int L, const int4* __restrict__ lvl, const uint8_t* __restrict__ cur, const uint8_t* __restrict__ forw,
                                                 const float* __restrict__ pts, float* __restrict__ out, uint8_t* __restrict__ status_out, uint8_t* __restrict__ codes,
                                                 uint8_t* __restrict__ iters) {
    __shared__ short s_i[VT_PATCH2], s_ix[VT_PATCH2], s_iy[VT_PATCH2];
    const int i = blockIdx.x, lane = threadIdx.x;
    if (n_dev) n = min(n, *n_dev);
    if (i >= n) return;
    const float ptx = pts[2 * i], pty = pts[2 * i + 1];
    int q[VT_PER_LANE];                                     // this lane's window positions in the staged patch; -1: none
#pragma unroll
    for (int j = 0; j < VT_PER_LANE; ++j) {
        const int k = lane + 64 * j, y = k / VTRACK_WIN;
        q[j] = k < VT_WIN2 ? y * VT_PATCH + (k - y * VTRACK_WIN) : -1;
    }
    float nx = 0.f, ny = 0.f;
    int status = 1;
    for (int l = L; l >= 0; --l) {
        const int4 lv = lvl[l];
        const int W = lv.x, H = lv.y;
        const uint8_t* I = cur + lv.z; const uint8_t* J = forw + lv.z;
        const float sc = 1.0f / (float)(1 << l);
        const float prx = ptx * sc, pry = pty * sc;
        if (l == L) { nx = prx; ny = pry; } else { nx = nx * 2.0f; ny = ny * 2.0f; }
        int code = VTRACK_CODE_SKIP, n_it = 0;
        const float px = prx - 10.0f, py = pry - 10.0f, fx = floorf(px), fy = floorf(py);
        if (!lk_inside(fx, fy, W, H)) {                                                             // step 3
            if (l == 0) status = 0;
        } else {
            const Weights w = weights(px - fx, py - fy);
            __syncthreads();                                                                        // the last level's reads of the patch are done
            lk_stage<true>(I, W, H, (int)fx, (int)fy, lane, s_i, s_ix, s_iy);
            __syncthreads();
            int Iw[VT_PER_LANE], Dx[VT_PER_LANE], Dy[VT_PER_LANE];                                  // step 4
            long long sxx = 0, sxy = 0, syy = 0;
#pragma unroll
            for (int j = 0; j < VT_PER_LANE; ++j) {
                Iw[j] = Dx[j] = Dy[j] = 0;
                if (q[j] >= 0) {
                    Iw[j] = lk_interp(s_i, q[j], w, 256, 9); Dx[j] = lk_interp(s_ix, q[j], w, 8192, 14); Dy[j] = lk_interp(s_iy, q[j], w, 8192, 14);
                }
                sxx += (long long)(Dx[j] * Dx[j]); sxy += (long long)(Dx[j] * Dy[j]); syy += (long long)(Dy[j] * Dy[j]);
            }
            const float s20 = 1.0f / 1048576.0f;
            const float A11 = (float)wave_sum(sxx) * s20, A12 = (float)wave_sum(sxy) * s20, A22 = (float)wave_sum(syy) * s20;
            float D = A11 * A22 - A12 * A12;
            const float dif = A11 - A22;
            const float min_eig = ((A22 + A11) - sqrtf(dif * dif + (4.0f * A12) * A12)) / 882.0f;
            if (min_eig < 1e-4f || D < FLT_EPSILON) {
                code = VTRACK_CODE_LOWEIG;
                if (l == 0) status = 0;
            } else {
                D = 1.0f / D;
                nx = nx - 10.0f; ny = ny - 10.0f;                                                  // step 5
                float dpx = 0.f, dpy = 0.f;
                code = VTRACK_CODE_CAP;
                for (int it = 0; it < VTRACK_MAX_ITERS; ++it) {
                    const float gx = floorf(nx), gy = floorf(ny);
                    if (!lk_inside(gx, gy, W, H)) {
                        code = VTRACK_CODE_OOB;
                        if (l == 0) status = 0;
                        break;
                    }
                    const Weights wj = weights(nx - gx, ny - gy);
                    __syncthreads();
                    lk_stage<false>(J, W, H, (int)gx, (int)gy, lane, s_i, nullptr, nullptr);
                    __syncthreads();
                    long long s1 = 0, s2 = 0;
#pragma unroll
                    for (int j = 0; j < VT_PER_LANE; ++j)
                        if (q[j] >= 0) {
                            const int diff = lk_interp(s_i, q[j], wj, 256, 9) - Iw[j];
                            s1 += (long long)(diff * Dx[j]); s2 += (long long)(diff * Dy[j]);
                        }
                    const float b1 = (float)wave_sum(s1) * s20, b2 = (float)wave_sum(s2) * s20;
                    const float dx = (A12 * b2 - A22 * b1) * D, dy = (A12 * b1 - A11 * b2) * D;
                    nx = nx + dx; ny = ny + dy;
                    n_it = it + 1;
                    if (dx * dx + dy * dy <= 1e-4f) { code = VTRACK_CODE_EPS; break; }
                    if (it > 0 && fabsf(dx + dpx) < 0.01f && fabsf(dy + dpy) < 0.01f) {
                        nx = nx - dx * 0.5f; ny = ny - dy * 0.5f;
                        code = VTRACK_CODE_OSC;
                        break;
                    }
                    dpx = dx; dpy = dy;
                }
                nx = nx + 10.0f; ny = ny + 10.0f;
            }
        }
        if (lane == 0) { codes[i * (L + 1) + l] = (uint8_t)code; iters[i * (L + 1) + l] = (uint8_t)n_it; }
    }
    if (lane == 0) {                                                                                // step 6
        const int4 l0 = lvl[0];
        const float rx = rintf(nx), ry = rintf(ny);
        const bool in = rx >= 1.0f && rx < (float)(l0.x - 1) && ry >= 1.0f && ry < (float)(l0.y - 1);
        out[2 * i] = nx; out[2 * i + 1] = ny;
        status_out[i] = (uint8_t)(status && in ? 1 : 0);
    }
}

// ---- step 7 ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(VT_ONE_WG) void k_track_mask(int n, const int* __restrict__ n_dev, const float* __restrict__ tracks, int md, int W, int H, uint8_t* __restrict__ kept,
                                                          int* __restrict__ hdr) {
    __shared__ int s_px[VTRACK_MAX_POINTS_LIMIT], s_py[VTRACK_MAX_POINTS_LIMIT];
    __shared__ volatile uint8_t s_st[VTRACK_MAX_POINTS_LIMIT];                                       // 0 undecided, 1 kept, 2 dropped
    __shared__ int s_kept;
    const int t = threadIdx.x;
    if (n_dev) n = min(n, *n_dev);                                                                   // the same in every thread
    if (t == 0) s_kept = 0;
    for (int i = t; i < n; i += VT_ONE_WG) {                                                         // n <= VTRACK_MAX_POINTS_LIMIT (checked by the host)
        const float rx = rintf(tracks[2 * i]), ry = rintf(tracks[2 * i + 1]);
        const bool in = rx >= 0.0f && rx < (float)W && ry >= 0.0f && ry < (float)H;
        s_px[i] = in ? (int)rx : 0; s_py[i] = in ? (int)ry : 0;
        s_st[i] = in ? 0 : 2;
    }
    __syncthreads();
    const int md2 = md * md;
    for (int round = 0; round < n + 2; ++round) {
        int pending = 0;
        for (int i = t; i < n; i += VT_ONE_WG) {
            if (s_st[i] != 0) continue;
            const int x = s_px[i], y = s_py[i];
            int ns = 1;
            for (int j = 0; j < i; ++j) {
                const int sj = s_st[j];
                if (sj == 2) continue;
                const int dx = s_px[j] - x, dy = s_py[j] - y;
                if (dx * dx + dy * dy <= md2) {
                    if (sj == 1) { ns = 2; break; }
                    ns = 0;
                }
            }
            if (ns) s_st[i] = (uint8_t)ns; else pending = 1;
        }
        const int any = __syncthreads_or(pending);
        if (!any) break;
        if (round == n + 1 && t == 0) hdr[H_FAIL] = 1;
    }
    for (int i = t; i < n; i += VT_ONE_WG) {
        const int k = s_st[i] == 1;
        kept[i] = (uint8_t)k;
        if (k) atomicAdd(&s_kept, 1);
    }
    __syncthreads();
    if (t == 0) hdr[H_NKEPT] = s_kept;
}

// the mask: a workgroup per track paints the disc of a kept one (every writer writes 0)
__global__ __launch_bounds__(256) void k_track_paint(const int* __restrict__ n_dev, const float* __restrict__ tracks, const uint8_t* __restrict__ kept, int md, int W, int H,
                                                   uint8_t* __restrict__ mask) {
    const int i = blockIdx.x;
    if (n_dev && i >= *n_dev) return;
    if (!kept[i]) return;                                                                           // kept: inside the image, so the casts are defined
    const int cx = (int)rintf(tracks[2 * i]), cy = (int)rintf(tracks[2 * i + 1]);
    const int side = 2 * md + 1, area = side * side, md2 = md * md;                                // md <= VTRACK_MAX_MIN_DIST: area < 2^23
    for (int k = threadIdx.x; k < area; k += 256) {
        const int ry = k / side, dx = k - ry * side - md, dy = ry - md;
        const int x = cx + dx, y = cy + dy;
        if (dx * dx + dy * dy <= md2 && x >= 0 && x < W && y >= 0 && y < H) mask[(size_t)y * W + x] = 0;
    }
}

// ---- step 8 ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_track_eig(const uint8_t* __restrict__ img, int W, int H, const uint8_t* __restrict__ mask, float* __restrict__ eig,
                                                   int* __restrict__ hdr) {
    __shared__ int s_xx[18 * 18], s_xy[18 * 18], s_yy[18 * 18];
    const int t = threadIdx.x, ox = blockIdx.x * 16, oy = blockIdx.y * 16;
    for (int k = t; k < 18 * 18; k += 256) {
        const int ty = k / 18, tx = k - ty * 18;
        const int u = r101(ox + tx - 1, W), v = r101(oy + ty - 1, H);                               // the pixel whose products the box reads there
        const int um = r101(u - 1, W), up = r101(u + 1, W);
        const uint8_t* rm = img + (size_t)r101(v - 1, H) * W; const uint8_t* r0 = img + (size_t)v * W; const uint8_t* rp = img + (size_t)r101(v + 1, H) * W;
        const int a = rm[um], b = rm[u], c = rm[up], d = r0[um], e = r0[up], f = rp[um], g = rp[u], h = rp[up];
        const int dx = (c + 2 * e + h) - (a + 2 * d + f), dy = (f + 2 * g + h) - (a + 2 * b + c);
        s_xx[k] = dx * dx; s_xy[k] = dx * dy; s_yy[k] = dy * dy;
    }
    __syncthreads();
    const int tx = t & 15, ty = t >> 4, x = ox + tx, y = oy + ty;
    unsigned bits = 0;
    if (x < W && y < H) {
        int sxx = 0, sxy = 0, syy = 0;
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int i = 0; i < 3; ++i) { const int k = (ty + j) * 18 + tx + i; sxx += s_xx[k]; sxy += s_xy[k]; syy += s_yy[k]; }
        const float s = 1.0f / 3060.0f;
        const float s2 = s * s;
        const float a = ((float)sxx * s2) * 0.5f, b = (float)sxy * s2, c = ((float)syy * s2) * 0.5f;
        const float d = a - c;
        const float e = (a + c) - sqrtf(d * d + b * b);
        const size_t p = (size_t)y * W + x;
        eig[p] = e;
        if (e > 0.0f && mask[p] == 255) bits = __float_as_uint(e);                                  // positive floats order like their bits
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) bits = max(bits, (unsigned)__shfl_xor((int)bits, o));
    if ((t & 63) == 0 && bits) atomicMax((unsigned*)&hdr[H_MAXBITS], bits);
}

// ---- step 9 ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_track_cand(const float* __restrict__ eig, const uint8_t* __restrict__ mask, int W, int H, float quality, int max_cand,
                                                    unsigned* __restrict__ candeig, unsigned long long* __restrict__ bitmap, int* __restrict__ cstate, int* __restrict__ clist,
                                                    int* __restrict__ hdr) {
    const int p = blockIdx.x * 256 + threadIdx.x;                                                   // a wave covers the 64 pixels of one bitmap word
    bool cand = false;
    float e = 0.f;
    if (p < W * H) {
        const int y = p / W, x = p - y * W;
        const float thr = __uint_as_float((unsigned)hdr[H_MAXBITS]) * quality;
        e = eig[p];
        cand = e > thr && mask[p] == 255 && x >= 1 && x < W - 1 && y >= 1 && y < H - 1;
        if (cand) {
#pragma unroll
            for (int j = -1; j <= 1; ++j)
#pragma unroll
                for (int i = -1; i <= 1; ++i) {
                    const float q = eig[(size_t)r101(y + j, H) * W + r101(x + i, W)];
                    if (q > thr && q > e) cand = false;                                             // e equals the maximum of the thresholded map
                }
        }
        candeig[p] = cand ? __float_as_uint(e) : 0u;                                                // a candidate's eig is > thr >= 0: its bits are not 0
        cstate[p] = 0;
        if (cand) {
            const int slot = atomicAdd(&hdr[H_NCAND], 1);                                           // the list's order is arbitrary; nothing depends on it
            if (slot < max_cand) clist[slot] = p;
        }
    }
    const unsigned long long b = __ballot(cand);                                                    // all 64 lanes get here
    if ((threadIdx.x & 63) == 0 && p < W * H) bitmap[p >> 6] = b;                                   // p >> 6 < ceil(W H / 64)
}

// ---- step 10 ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool outranks(const unsigned eq, const int q, const unsigned e, const int p) { return eq > e || (eq == e && q < p); }

__device__ __forceinline__ int state_of(const int* cstate, const int p) { return __hip_atomic_load(&cstate[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// A wave decides candidate p from the states as they are: 1 picked (no undropped candidate of higher rank within the disc), 2 dropped (a picked
// one there), 0 still undecided.  A lane takes a row of the disc: the chord's pixels are a run of bits in the candidate bitmap, so it reads the
// words of the run and visits the set bits only.  Wave-uniform result.
__device__ __forceinline__ int pick_visit(const int p, const int lane, const int W, const int H, const int md, const unsigned* __restrict__ candeig,
                                          const unsigned long long* __restrict__ bitmap, const int* cstate) {
    if (md <= 0) return 1;
    const unsigned e = candeig[p];
    const int y = p / W, x = p - y * W, r = md - 1, side = 2 * r + 1, md2 = md * md;
    int ns = 1;
    for (int rb = 0; rb < side; rb += 64) {
        const int dy = rb + lane - r, yy = y + dy;
        int mine = 1;
        if (rb + lane < side && yy >= 0 && yy < H) {
            int hw = (int)sqrtf((float)(md2 - 1 - dy * dy));                                        // the largest dx with dx^2 + dy^2 < md^2; |dy| <= md - 1
            while ((hw + 1) * (hw + 1) + dy * dy < md2) ++hw;
            while (hw > 0 && hw * hw + dy * dy >= md2) --hw;
            const int a = yy * W + max(0, x - hw), b = yy * W + min(W - 1, x + hw);                 // pixel indices inside the image
            for (int w = a >> 6; w <= (b >> 6) && mine != 2; ++w) {
                unsigned long long bits = bitmap[w];
                if (w == (a >> 6)) bits &= ~0ull << (a & 63);
                if (w == (b >> 6)) bits &= ~0ull >> (63 - (b & 63));
                while (bits) {
                    const int qi = w * 64 + __builtin_ctzll(bits);
                    bits &= bits - 1;
                    if (qi == p) continue;
                    if (outranks(candeig[qi], qi, e, p)) {
                        const int sq = state_of(cstate, qi);
                        if (sq == 1) { mine = 2; break; }
                        if (sq == 0) mine = 0;
                    }
                }
            }
        }
        if (__any(mine == 2)) return 2;
        if (__any(mine == 0)) ns = 0;
    }
    return ns;
}

// the same as a call: inlined into k_track_pick's loops it costs that kernel six spilled scalar registers
__device__ __noinline__ int pick_visit_call(const int p, const int lane, const int W, const int H, const int md, const unsigned* __restrict__ candeig,
                                            const unsigned long long* __restrict__ bitmap, const int* cstate) {
    return pick_visit(p, lane, W, H, md, candeig, bitmap, cstate);
}

// one round of the fixpoint over all candidates on the whole device; VT_ROUNDS of them run before k_track_pick finishes what is left
__global__ __launch_bounds__(256) void k_track_round(int W, int H, int md, int max_cand, const unsigned* __restrict__ candeig, const unsigned long long* __restrict__ bitmap,
                                                     int* cstate, const int* __restrict__ clist, const int* __restrict__ hdr) {
    const int lane = threadIdx.x & 63, nc = hdr[H_NCAND];
    if (nc > max_cand) return;
    for (int k = blockIdx.x * 4 + (threadIdx.x >> 6); k < nc; k += gridDim.x * 4) {                  // k < nc <= max_cand
        const int p = clist[k];
        if (state_of(cstate, p) != 0) continue;
        const int ns = pick_visit(p, lane, W, H, md, candeig, bitmap, cstate);
        if (ns && lane == 0) __hip_atomic_store(&cstate[p], ns, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(VT_ONE_WG) void k_track_pick(int W, int H, int md, int max_cnt, int max_cand, const unsigned* __restrict__ candeig,
                                                          const unsigned long long* __restrict__ bitmap, int* cstate, const int* __restrict__ clist, int* __restrict__ ulist,
                                                          int* __restrict__ plist, float* __restrict__ new_xy, int* __restrict__ hdr) {
    __shared__ int s_n, s_u;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int nc = hdr[H_NCAND];
    if (nc > max_cand) return;                                                                      // the host returns VIL_ERR_UNSUPPORTED
    if (t == 0) { s_n = 0; s_u = 0; }
    __syncthreads();
    for (int k = t; k < nc; k += VT_ONE_WG) {                                                        // what the rounds before left undecided
        const int p = clist[k];
        if (state_of(cstate, p) == 0) ulist[atomicAdd(&s_u, 1)] = p;                                // at most nc <= max_cand entries
    }
    __syncthreads();
    const int nu = s_u;
    int rounds = 0;
    for (int round = 0; nu && round < nu + 2; ++round) {
        int pending = 0;
        for (int k = wave; k < nu; k += VT_ONE_WG / 64) {
            const int p = ulist[k];
            if (state_of(cstate, p) != 0) continue;
            const int ns = pick_visit_call(p, lane, W, H, md, candeig, bitmap, cstate);
            if (ns) { if (lane == 0) __hip_atomic_store(&cstate[p], ns, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
            else pending = 1;
        }
        rounds = round + 1;
        const int any = __syncthreads_or(pending);
        if (!any) break;
        if (round == nu + 1 && t == 0) hdr[H_FAIL] = 1;
    }
    for (int k = t; k < nc; k += VT_ONE_WG) {
        const int p = clist[k];
        if (state_of(cstate, p) == 1) plist[atomicAdd(&s_n, 1)] = p;                                // at most nc <= max_cand entries
    }
    __syncthreads();
    const int np = s_n, need = max(0, max_cnt - hdr[H_NKEPT]);
    for (int k = t; k < np; k += VT_ONE_WG) {
        const int p = plist[k];
        const unsigned e = candeig[p];
        int rank = 0;
        for (int j = 0; j < np; ++j) { const int qj = plist[j]; rank += outranks(candeig[qj], qj, e, p) ? 1 : 0; }
        if (rank < need) { const int y = p / W; new_xy[2 * rank] = (float)(p - y * W); new_xy[2 * rank + 1] = (float)y; }       // rank < need <= max_cnt, rank < np <= max_cand
    }
    if (t == 0) { hdr[H_NPICK] = np; hdr[H_NNEW] = min(np, need); hdr[H_ROUNDS] = VT_ROUNDS + rounds; }
}

}  // namespace

struct vtrack_ctx : vilhost::Device {        // d_mem: pyramid slot 0 | slot 1 | level table | points | forw_xy, status | codes | iters | counters, kept, new_xy | maps | lists
    vtrack_cfg cfg = {};
    int lw[VTRACK_MAX_LEVEL + 1] = {}, lh[VTRACK_MAX_LEVEL + 1] = {};
    size_t loff[VTRACK_MAX_LEVEL + 1] = {}, slot_bytes = 0;
    int n_images = 0, forw = 0, cur = 0;                    // slots of the two images; n_images saturates at 2
    int last_n = 0; bool detected = false;                  // what vtrack_debug_read reads
    char* h_img = nullptr; char* h_in = nullptr; char* h_out = nullptr;
    size_t o_slot[2] = {}, o_lvl = 0, o_pts = 0, o_forw = 0, o_status = 0, o_codes = 0, o_iters = 0, o_hdr = 0, o_kept = 0, o_new = 0, o_eig = 0, o_mask = 0, o_candeig = 0,
           o_cstate = 0, o_bitmap = 0, o_clist = 0, o_ulist = 0, o_plist = 0;
    vilhost::Profiler<VTRACK_NUM_KERNELS, 8> prof;
};

// ---- the stages of vtrack_push_image (viltrack_stage.hpp) ------------------------------------------------------------------------
// the slot the next image goes to: never the slot of the image that becomes cur
static int next_slot(const vtrack_ctx* c) { return c->n_images ? 1 - c->forw : 0; }

viltrack_stage::Target viltrack_stage::target(const vtrack_ctx* c) {
    return {(uint8_t*)(c->d_mem + c->o_slot[next_slot(c)] + c->loff[0]), c->stream, c->device, c->cfg.width, c->cfg.height};
}

const uint8_t* viltrack_stage::stage_image(vtrack_ctx* c, const uint8_t* gray, const int row_stride) {
    const int W = c->cfg.width, H = c->cfg.height;
    for (int y = 0; y < H; ++y) memcpy(c->h_img + (size_t)y * W, gray + (size_t)y * row_stride, W);
    return (const uint8_t*)c->h_img;
}

int viltrack_stage::enqueue_push(vtrack_ctx* c) {
    const int L = c->cfg.max_level, slot = next_slot(c);
    uint8_t* base = (uint8_t*)(c->d_mem + c->o_slot[slot]);
    for (int l = 0; l < L; ++l) {
        VILCHK(c->prof.mark(l, c->stream));
        const int n2 = c->lw[l + 1] * c->lh[l + 1];
        hipLaunchKernelGGL(k_track_pyr, dim3((n2 + 255) / 256), dim3(256), 0, c->stream, base + c->loff[l], c->lw[l], c->lh[l], base + c->loff[l + 1], c->lw[l + 1], c->lh[l + 1]);
    }
    VILCHK(c->prof.mark(L, c->stream));
    return VIL_OK;
}

void viltrack_stage::commit_push(vtrack_ctx* c) {
    const int slot = next_slot(c);
    c->cur = c->n_images ? c->forw : slot; c->forw = slot;
    if (c->n_images < 2) c->n_images++;
}

int viltrack_stage::finish_push(vtrack_ctx* c) {
    const int st = enqueue_push(c);
    if (st != VIL_OK) return st;
    VILCHK(hipStreamSynchronize(c->stream));
    VILCHK(hipGetLastError());
    for (int l = 0; l < c->cfg.max_level; ++l) c->prof.span(0, l, l + 1);
    commit_push(c);
    return VIL_OK;
}

void viltrack_stage::forget(vtrack_ctx* c) { c->n_images = 0; c->forw = c->cur = 0; }

int viltrack_stage::enqueue_lk(vtrack_ctx* c, const int n_max, const int* d_n, const float* d_pts, float* d_forw, uint8_t* d_status) {
    char* d = c->d_mem;
    VILCHK(c->prof.mark(0, c->stream));
    hipLaunchKernelGGL(k_track_lk, dim3(n_max), dim3(64), 0, c->stream, n_max, d_n, c->cfg.max_level, (const int4*)(d + c->o_lvl), (const uint8_t*)(d + c->o_slot[c->cur]),
                       (const uint8_t*)(d + c->o_slot[c->forw]), d_pts, d_forw, d_status, (uint8_t*)(d + c->o_codes), (uint8_t*)(d + c->o_iters));
    VILCHK(c->prof.mark(1, c->stream));
    return VIL_OK;
}

int viltrack_stage::enqueue_detect(vtrack_ctx* c, const int n_max, const int* d_n, const float* d_pts, const int min_dist, const int max_cnt, const float quality,
                                   Detection* out) {
    char* d = c->d_mem;
    const int W = c->cfg.width, H = c->cfg.height, MC = c->cfg.max_candidates;
    const size_t WH = (size_t)W * H;
    const uint8_t* img = (const uint8_t*)(d + c->o_slot[c->forw]);
    int* d_hdr = (int*)(d + c->o_hdr); uint8_t* d_mask = (uint8_t*)(d + c->o_mask); float* d_eig = (float*)(d + c->o_eig);
    unsigned* d_candeig = (unsigned*)(d + c->o_candeig); int* d_cstate = (int*)(d + c->o_cstate); int* d_clist = (int*)(d + c->o_clist);
    VILCHK(hipMemsetAsync(d_hdr, 0, 4 * H_INTS, c->stream));
    VILCHK(hipMemsetAsync(d_mask, 255, WH, c->stream));
    unsigned long long* d_bitmap = (unsigned long long*)(d + c->o_bitmap); uint8_t* d_kept = (uint8_t*)(d + c->o_kept);
    VILCHK(c->prof.mark(0, c->stream));
    hipLaunchKernelGGL(k_track_mask, dim3(1), dim3(VT_ONE_WG), 0, c->stream, n_max, d_n, d_pts, min_dist, W, H, d_kept, d_hdr);
    VILCHK(c->prof.mark(1, c->stream));
    if (n_max) hipLaunchKernelGGL(k_track_paint, dim3(n_max), dim3(256), 0, c->stream, d_n, d_pts, d_kept, min_dist, W, H, d_mask);
    VILCHK(c->prof.mark(2, c->stream));
    hipLaunchKernelGGL(k_track_eig, dim3((W + 15) / 16, (H + 15) / 16), dim3(256), 0, c->stream, img, W, H, d_mask, d_eig, d_hdr);
    VILCHK(c->prof.mark(3, c->stream));
    hipLaunchKernelGGL(k_track_cand, dim3((unsigned)((WH + 255) / 256)), dim3(256), 0, c->stream, d_eig, d_mask, W, H, quality, MC, d_candeig, d_bitmap, d_cstate, d_clist, d_hdr);
    VILCHK(c->prof.mark(4, c->stream));
    for (int k = 0; k < VT_ROUNDS; ++k)
        hipLaunchKernelGGL(k_track_round, dim3(std::min(1024, (MC + 3) / 4)), dim3(256), 0, c->stream, W, H, min_dist, MC, d_candeig, d_bitmap, d_cstate, d_clist, d_hdr);
    VILCHK(c->prof.mark(5, c->stream));
    hipLaunchKernelGGL(k_track_pick, dim3(1), dim3(VT_ONE_WG), 0, c->stream, W, H, min_dist, max_cnt, MC, d_candeig, d_bitmap, d_cstate, d_clist, (int*)(d + c->o_ulist),
                       (int*)(d + c->o_plist), (float*)(d + c->o_new), d_hdr);
    VILCHK(c->prof.mark(6, c->stream));
    if (out) *out = {d_hdr, d_kept, (float*)(d + c->o_new)};
    return VIL_OK;
}

extern "C" {

int vtrack_create(int32_t device, const vtrack_cfg* cfg, vtrack_ctx** out) {
    if (!out || !cfg || cfg->width < 16 || cfg->width > 16384 || cfg->height < 16 || cfg->height > 16384 || cfg->max_level < 0 || cfg->max_level > VTRACK_MAX_LEVEL ||
        cfg->max_points < 1 || cfg->max_points > VTRACK_MAX_POINTS_LIMIT || cfg->max_candidates < 1)
        return VIL_ERR_INVALID_ARGUMENT;
    vtrack_ctx* c = new vtrack_ctx();
    c->cfg = *cfg;
    const size_t WH = (size_t)cfg->width * cfg->height, P = (size_t)cfg->max_points;
    if ((size_t)c->cfg.max_candidates > WH) c->cfg.max_candidates = (int)WH;                         // there are no more pixels than that
    const size_t MC = (size_t)c->cfg.max_candidates;
    vilhost::Arena a, s;
    for (int l = 0; l <= cfg->max_level; ++l) {
        c->lw[l] = l ? (c->lw[l - 1] + 1) / 2 : cfg->width; c->lh[l] = l ? (c->lh[l - 1] + 1) / 2 : cfg->height;
        c->loff[l] = s.take((size_t)c->lw[l] * c->lh[l]);
    }
    c->slot_bytes = s.bytes;
    c->o_slot[0] = a.take(s.bytes); c->o_slot[1] = a.take(s.bytes);
    c->o_lvl = a.take(16 * (VTRACK_MAX_LEVEL + 1));
    c->o_pts = a.take(8 * P);
    c->o_forw = a.take(8 * P); c->o_status = a.take(P);     // read back together
    c->o_codes = a.take(P * (VTRACK_MAX_LEVEL + 1)); c->o_iters = a.take(P * (VTRACK_MAX_LEVEL + 1));
    c->o_hdr = a.take(4 * H_INTS); c->o_kept = a.take(P); c->o_new = a.take(8 * MC);               // read back together
    c->o_eig = a.take(4 * WH); c->o_mask = a.take(WH); c->o_candeig = a.take(4 * WH); c->o_cstate = a.take(4 * WH);
    c->o_bitmap = a.take(8 * ((WH + 63) / 64));
    c->o_clist = a.take(4 * MC); c->o_ulist = a.take(4 * MC); c->o_plist = a.take(4 * MC);
    hipError_t err = c->open(device, a.bytes);
    if (err == hipSuccess) err = c->pin(&c->h_img, vilhost::up16(WH));
    if (err == hipSuccess) err = c->pin(&c->h_in, std::max((size_t)(16 * (VTRACK_MAX_LEVEL + 1)), vilhost::up16(8 * P)));      // also stages the level table
    if (err == hipSuccess) err = c->pin(&c->h_out, std::max(c->o_codes - c->o_forw, c->o_eig - c->o_hdr));
    if (err == hipSuccess) {
        int4* t = (int4*)c->h_in;
        for (int l = 0; l <= VTRACK_MAX_LEVEL; ++l) t[l] = l <= cfg->max_level ? make_int4(c->lw[l], c->lh[l], (int)c->loff[l], 0) : make_int4(1, 1, 0, 0);
        err = hipMemsetAsync(c->d_mem, 0, a.bytes, c->stream);
        if (err == hipSuccess) err = hipMemcpyAsync(c->d_mem + c->o_lvl, t, 16 * (VTRACK_MAX_LEVEL + 1), hipMemcpyHostToDevice, c->stream);
        if (err == hipSuccess) err = hipStreamSynchronize(c->stream);
    }
    if (err != hipSuccess) { vtrack_destroy(c); VILCHK(err); }
    *out = c;
    return VIL_OK;
}

void vtrack_destroy(vtrack_ctx* c) {
    if (!c) return;
    c->close(c->prof);
    delete c;
}

int vtrack_profile_enable(vtrack_ctx* c, int32_t enable) {
    if (!c) return VIL_ERR_INVALID_ARGUMENT;
    VILCHK(c->prof.enable(c->device, enable != 0));
    return VIL_OK;
}
int vtrack_profile_read(vtrack_ctx* c, int64_t* launches8, double* total_ms8) {
    if (!c || !launches8 || !total_ms8) return VIL_ERR_INVALID_ARGUMENT;
    c->prof.read(launches8, total_ms8);
    return VIL_OK;
}

int vtrack_push_image(vtrack_ctx* c, const uint8_t* gray, int32_t row_stride) {
    if (!c || !gray || row_stride < c->cfg.width) return VIL_ERR_INVALID_ARGUMENT;
    VILCHK(hipSetDevice(c->device));
    const uint8_t* staged = viltrack_stage::stage_image(c, gray, row_stride);
    VILCHK(hipMemcpyAsync(viltrack_stage::target(c).level0, staged, (size_t)c->cfg.width * c->cfg.height, hipMemcpyHostToDevice, c->stream));
    return viltrack_stage::finish_push(c);
}

int vtrack_track(vtrack_ctx* c, int32_t n, const float* cur_xy, float* forw_xy, uint8_t* status, vtrack_summary* out) {
    if (!c || n < 0 || n > c->cfg.max_points || !c->n_images || (n && (!cur_xy || !forw_xy || !status))) return VIL_ERR_INVALID_ARGUMENT;
    int tracked = 0;
    if (n) {
        VILCHK(hipSetDevice(c->device));
        char* d = c->d_mem;
        memcpy(c->h_in, cur_xy, 8 * (size_t)n);
        VILCHK(hipMemcpyAsync(d + c->o_pts, c->h_in, 8 * (size_t)n, hipMemcpyHostToDevice, c->stream));
        const int st = viltrack_stage::enqueue_lk(c, n, nullptr, (const float*)(d + c->o_pts), (float*)(d + c->o_forw), (uint8_t*)(d + c->o_status));
        if (st != VIL_OK) return st;
        const size_t st_off = c->o_status - c->o_forw;
        VILCHK(hipMemcpyAsync(c->h_out, d + c->o_forw, st_off + (size_t)n, hipMemcpyDeviceToHost, c->stream));
        VILCHK(hipStreamSynchronize(c->stream));
        VILCHK(hipGetLastError());
        c->prof.span(1, 0, 1);
        memcpy(forw_xy, c->h_out, 8 * (size_t)n); memcpy(status, c->h_out + st_off, (size_t)n);
        for (int i = 0; i < n; ++i) tracked += status[i];
    }
    c->last_n = n;
    if (out) { memset(out, 0, sizeof *out); out->n_points = n; out->n_tracked = tracked; }
    return VIL_OK;
}

int vtrack_detect(vtrack_ctx* c, int32_t n_tracks, const float* tracks_xy, int32_t min_dist, int32_t max_cnt, float quality, uint8_t* kept, int32_t* n_new, float* new_xy,
                  vtrack_summary* out) {
    if (!c || n_tracks < 0 || n_tracks > c->cfg.max_points || !c->n_images || (n_tracks && (!tracks_xy || !kept)) || !n_new || (max_cnt > 0 && !new_xy) || min_dist < 0 ||
        min_dist > VTRACK_MAX_MIN_DIST || max_cnt < 0 || !(quality > 0.0f && quality <= 1.0f))
        return VIL_ERR_INVALID_ARGUMENT;
    VILCHK(hipSetDevice(c->device));
    char* d = c->d_mem;
    const int MC = c->cfg.max_candidates;
    int* d_hdr = (int*)(d + c->o_hdr);
    if (n_tracks) {
        memcpy(c->h_in, tracks_xy, 8 * (size_t)n_tracks);
        VILCHK(hipMemcpyAsync(d + c->o_pts, c->h_in, 8 * (size_t)n_tracks, hipMemcpyHostToDevice, c->stream));
    }
    const int st = viltrack_stage::enqueue_detect(c, n_tracks, nullptr, (const float*)(d + c->o_pts), min_dist, max_cnt, quality, nullptr);
    if (st != VIL_OK) return st;
    const size_t kept_off = c->o_kept - c->o_hdr, new_off = c->o_new - c->o_hdr;
    VILCHK(hipMemcpyAsync(c->h_out, d_hdr, new_off + 8 * (size_t)std::min(max_cnt, MC), hipMemcpyDeviceToHost, c->stream));
    VILCHK(hipStreamSynchronize(c->stream));
    VILCHK(hipGetLastError());
    for (int k = 0; k < 6; ++k) if (k != 1 || n_tracks) c->prof.span(2 + k, k, k + 1);
    if (c->prof.on) c->prof.n[6] += VT_ROUNDS - 1;                                                 // the span of k_track_round holds VT_ROUNDS launches
    c->detected = true;
    const int* hdr = (const int*)c->h_out;
    if (hdr[H_FAIL]) return VIL_ERR_DEVICE;
    if (hdr[H_NCAND] > MC) return VIL_ERR_UNSUPPORTED;                                             // before any output is written
    if (n_tracks) memcpy(kept, c->h_out + kept_off, (size_t)n_tracks);
    *n_new = hdr[H_NNEW];
    if (hdr[H_NNEW]) memcpy(new_xy, c->h_out + new_off, 8 * (size_t)hdr[H_NNEW]);
    if (out) {
        memset(out, 0, sizeof *out);
        out->n_tracks = n_tracks; out->n_kept = hdr[H_NKEPT]; out->n_candidates = hdr[H_NCAND]; out->n_picked = hdr[H_NPICK]; out->n_new = hdr[H_NNEW]; out->rounds = hdr[H_ROUNDS];
    }
    return VIL_OK;
}

int vtrack_debug_read(vtrack_ctx* c, int32_t what, int32_t arg, void* dst, int64_t capacity_bytes) {
    if (!c || !dst) return VIL_ERR_INVALID_ARGUMENT;
    const size_t WH = (size_t)c->cfg.width * c->cfg.height;
    size_t off = 0, bytes = 0;
    switch (what) {
    case VTRACK_DBG_CUR_LEVEL: case VTRACK_DBG_FORW_LEVEL:
        if (arg < 0 || arg > c->cfg.max_level || !c->n_images) return VIL_ERR_INVALID_ARGUMENT;
        off = c->o_slot[what == VTRACK_DBG_CUR_LEVEL ? c->cur : c->forw] + c->loff[arg]; bytes = (size_t)c->lw[arg] * c->lh[arg];
        break;
    case VTRACK_DBG_LK_CODES: off = c->o_codes; bytes = (size_t)c->last_n * (c->cfg.max_level + 1); break;
    case VTRACK_DBG_LK_ITERS: off = c->o_iters; bytes = (size_t)c->last_n * (c->cfg.max_level + 1); break;
    case VTRACK_DBG_EIG: off = c->o_eig; bytes = 4 * WH; break;
    case VTRACK_DBG_MASK: off = c->o_mask; bytes = WH; break;
    case VTRACK_DBG_N_CANDIDATES: off = c->o_hdr + 4 * H_NCAND; bytes = 4; break;
    default: return VIL_ERR_INVALID_ARGUMENT;
    }
    if (what >= VTRACK_DBG_EIG && !c->detected) return VIL_ERR_INVALID_ARGUMENT;
    if (capacity_bytes < (int64_t)bytes) return VIL_ERR_INVALID_ARGUMENT;
    if (!bytes) return VIL_OK;
    VILCHK(hipSetDevice(c->device));
    VILCHK(hipMemcpyAsync(dst, c->d_mem + off, bytes, hipMemcpyDeviceToHost, c->stream));
    VILCHK(hipStreamSynchronize(c->stream));
    return VIL_OK;
}

}  // extern "C"
