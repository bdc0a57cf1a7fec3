// vilclahe.hip -- CLAHE on gfx950 behind include/vilclahe.h (feature_tracker_/src/feature_tracker.cpp:87-93; the steps are numbered as
// in the header).
//
// Every entry point is one submission with one synchronisation; vclahe_push puts its launches into the tracker's stream, in front of the
// tracker's own k_track_pyr launches (viltrack_stage.hpp), and writes the equalised image straight into the tracker's level 0.
//   k_clahe_hist   step 3's histogram.  A tile is split into shares of about VC_SHARE pixels, a workgroup of 4 waves per share, so that a
//                  640 x 480 image at 8 x 8 tiles is 320 workgroups and not 64.  A thread reads a pixel of the extended image through
//                  r101 and adds to ITS WAVE's sub-histogram in LDS; a wave whose 64 pixels are all equal (a flat or saturated tile,
//                  where 64 adds to one address would serialise) adds 64 once.  The four sub-histograms are summed and the non-zero bins
//                  added to the tile's histogram in memory with integer atomics: exact in any order.
//   k_clahe_lut    a wave per tile, four adjacent bins per lane: the clipped excess is a wave reduction, the redistribution is step 3's
//                  closed form, the prefix sum is four bins in the lane and a shuffle scan across the lanes.  Writes the LUT and the
//                  histogram as redistributed (vclahe_debug_read).
//   k_clahe_blend  step 4, a thread per 4 adjacent pixels of a row: one 4-byte load and one 4-byte store per destination when width is a
//                  multiple of 4, bytes otherwise.  The LUTs (at most 64 kB) are read from memory: they stay in the caches.  Writes up
//                  to two destinations in the same pass (the tracker's level 0 and the image that is read back).
// The launches are separated by kernel boundaries; nothing is handed from one workgroup to another inside a launch.
// The float arithmetic of the contract is unfused and in source order (numpy does not contract a * b + c; hipcc would):
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/vilclahe.h"
#include "vil_host.hpp"
#include "vilclahe_stage.hpp"
#include "viltrack_stage.hpp"

#define VC_SHARE 1024                     // pixels of a tile that a workgroup of k_clahe_hist takes, at least
#define VC_MAX_SHARES 1024                // shares per tile, at most: beyond that a share grows

namespace {

__device__ __forceinline__ int r101(int i, const int n) {
    if ((unsigned)i < (unsigned)n) return i;
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    i %= p;
    if (i < 0) i += p;
    return i >= n ? p - i : i;                                                                      // in [0, n)
}

__device__ __forceinline__ uint8_t sat_u8(const float r) { return (uint8_t)fminf(fmaxf(r, 0.0f), 255.0f); }        // r is integral

// ---- step 3: the histogram -------------------------------------------------------------------------------------------------------
// grid (shares, tiles); share s of a tile is the pixels [s * chunk, min(area, (s + 1) * chunk)) of the tile in row order
__global__ __launch_bounds__(256) void k_clahe_hist(const uint8_t* __restrict__ src, int W, int H, int tw, int th, int tiles_x, int chunk, int* __restrict__ hist) {
    __shared__ int s_h[4][256];
    const int t = threadIdx.x, wave = t >> 6, tile = blockIdx.y;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x, ox = tx * tw, oy = ty * th;
#pragma unroll
    for (int w = 0; w < 4; ++w) s_h[w][t] = 0;
    __syncthreads();
    const int area = tw * th, k0 = (int)blockIdx.x * chunk, k1 = min(area, k0 + chunk);             // shares * chunk < 2^31 (the host)
    for (int kb = k0; kb < k1; kb += 256) {                                                         // wave-uniform bounds
        const int k = kb + t;
        int v = -1;
        if (k < k1) {
            const int py = k / tw, px = k - py * tw;
            v = src[(size_t)r101(oy + py, H) * W + r101(ox + px, W)];                               // inside the image
        }
        const int v0 = __builtin_amdgcn_readfirstlane(v);
        if (__all(v == v0)) {                                                                       // 64 equal pixels, or none at all
            if ((t & 63) == 0 && v0 >= 0) atomicAdd(&s_h[wave][v0], 64);
        } else if (v >= 0) {
            atomicAdd(&s_h[wave][v], 1);
        }
    }
    __syncthreads();
    const int sum = (s_h[0][t] + s_h[1][t]) + (s_h[2][t] + s_h[3][t]);
    if (sum) atomicAdd(&hist[tile * 256 + t], sum);                                                 // tile < tiles: 256 bins each
}

// ---- step 3: clip, redistribution, prefix sum, LUT -------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_clahe_lut(int* __restrict__ hist, uint8_t* __restrict__ lut, int clip, float lut_scale) {
    const int lane = threadIdx.x, tile = blockIdx.x;
    int4* hp = (int4*)(hist + tile * 256) + lane;                                                   // bins 4 lane .. 4 lane + 3
    const int4 h = *hp;
    int b[4] = {h.x, h.y, h.z, h.w};
    if (clip > 0) {
        int clipped = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) { clipped += max(b[j] - clip, 0); b[j] = min(b[j], clip); }
#pragma unroll
        for (int o = 32; o; o >>= 1) clipped += __shfl_xor(clipped, o);
        const int batch = clipped / 256, residual = clipped - 256 * batch;
        const int step = residual > 0 ? max(256 / residual, 1) : 1;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = 4 * lane + j;
            b[j] += batch + (residual > 0 && i % step == 0 && i / step < residual ? 1 : 0);
        }
    }
    *hp = make_int4(b[0], b[1], b[2], b[3]);
    const int mine = (b[0] + b[1]) + (b[2] + b[3]);
    int incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int up = __shfl_up(incl, o); if (lane >= o) incl += up; }
    int run = incl - mine;
    unsigned packed = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        run += b[j];
        packed |= (unsigned)sat_u8(rintf((float)run * lut_scale)) << (8 * j);
    }
    ((unsigned*)(lut + tile * 256))[lane] = packed;
}

// ---- step 4 ----------------------------------------------------------------------------------------------------------------------
struct Axis { int t1, t2; float a, a1; };
__device__ __forceinline__ Axis axis(const int x, const float inv, const int tiles) {
    const float tf = (float)x * inv - 0.5f, fl = floorf(tf);
    Axis r;
    r.a = tf - fl; r.a1 = 1.0f - r.a;
    const int t1 = (int)fl;                                                                         // >= -1
    r.t2 = min(t1 + 1, tiles - 1); r.t1 = max(t1, 0);
    return r;
}

// a thread per `groups`-th of a row: the pixels x0 .. x0 + 3.  vec: W % 4 == 0, every group is whole and 4-byte aligned in src, dst, dst2
__global__ __launch_bounds__(256) void k_clahe_blend(const uint8_t* __restrict__ src, int W, int H, int groups, int vec, const uint8_t* __restrict__ lut, int tiles_x,
                                                     int tiles_y, float inv_tw, float inv_th, uint8_t* __restrict__ dst, uint8_t* __restrict__ dst2) {
    const int g = blockIdx.x * 256 + threadIdx.x;                                                   // H * groups <= 2^26
    if (g >= H * groups) return;
    const int y = g / groups, x0 = (g - y * groups) * 4;
    const size_t p = (size_t)y * W + x0;
    const Axis ay = axis(y, inv_th, tiles_y);
    const uint8_t* l1 = lut + (size_t)ay.t1 * tiles_x * 256; const uint8_t* l2 = lut + (size_t)ay.t2 * tiles_x * 256;
    unsigned in = 0;
    if (vec) in = *(const unsigned*)(src + p);
    else
#pragma unroll
        for (int j = 0; j < 4; ++j) if (x0 + j < W) in |= (unsigned)src[p + j] << (8 * j);
    unsigned out = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int v = (in >> (8 * j)) & 255;
        const Axis ax = axis(min(x0 + j, W - 1), inv_tw, tiles_x);
        const int c1 = ax.t1 * 256 + v, c2 = ax.t2 * 256 + v;
        const float r = ((float)l1[c1] * ax.a1 + (float)l1[c2] * ax.a) * ay.a1 + ((float)l2[c1] * ax.a1 + (float)l2[c2] * ax.a) * ay.a;
        out |= (unsigned)sat_u8(rintf(r)) << (8 * j);
    }
    if (vec) {
        *(unsigned*)(dst + p) = out;
        if (dst2) *(unsigned*)(dst2 + p) = out;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (x0 + j < W) {
                dst[p + j] = (uint8_t)(out >> (8 * j));
                if (dst2) dst2[p + j] = (uint8_t)(out >> (8 * j));
            }
    }
}

}  // namespace

struct vclahe_ctx : vilhost::Device {        // d_mem: histograms | LUTs | the raw image | the equalised image
    vclahe_cfg cfg = {};
    int tw = 0, th = 0, clip = 0, shares = 0, chunk = 0;
    float lut_scale = 0.f, inv_tw = 0.f, inv_th = 0.f;
    bool ran = false;                                       // what vclahe_debug_read reads exists
    char* h_img = nullptr; char* h_out = nullptr;
    size_t o_hist = 0, o_lut = 0, o_src = 0, o_out = 0;
    vilhost::Profiler<VCLAHE_NUM_KERNELS, 4> prof;
};

// ---- the stages (vilclahe_stage.hpp) ---------------------------------------------------------------------------------------------
vilclahe_stage::Staged vilclahe_stage::stage_image(vclahe_ctx* c, const uint8_t* gray, const int row_stride) {
    const int W = c->cfg.width, H = c->cfg.height;
    for (int y = 0; y < H; ++y) memcpy(c->h_img + (size_t)y * W, gray + (size_t)y * row_stride, W);
    return {(const uint8_t*)c->h_img, (uint8_t*)(c->d_mem + c->o_src)};
}

int vilclahe_stage::enqueue_kernels(vclahe_ctx* c, hipStream_t stream, uint8_t* dst, uint8_t* dst2) {
    const int W = c->cfg.width, H = c->cfg.height, tiles = c->cfg.tiles_x * c->cfg.tiles_y, groups = (W + 3) / 4;
    char* d = c->d_mem;
    VILCHK(hipMemsetAsync(d + c->o_hist, 0, (size_t)tiles * 1024, stream));
    const uint8_t* src = (const uint8_t*)(d + c->o_src);
    VILCHK(c->prof.mark(0, stream));
    hipLaunchKernelGGL(k_clahe_hist, dim3(c->shares, tiles), dim3(256), 0, stream, src, W, H, c->tw, c->th, c->cfg.tiles_x, c->chunk, (int*)(d + c->o_hist));
    VILCHK(c->prof.mark(1, stream));
    hipLaunchKernelGGL(k_clahe_lut, dim3(tiles), dim3(64), 0, stream, (int*)(d + c->o_hist), (uint8_t*)(d + c->o_lut), c->clip, c->lut_scale);
    VILCHK(c->prof.mark(2, stream));
    hipLaunchKernelGGL(k_clahe_blend, dim3((H * groups + 255) / 256), dim3(256), 0, stream, src, W, H, groups, W % 4 == 0 ? 1 : 0, (const uint8_t*)(d + c->o_lut),
                       c->cfg.tiles_x, c->cfg.tiles_y, c->inv_tw, c->inv_th, dst, dst2);
    VILCHK(c->prof.mark(3, stream));
    return VIL_OK;
}

// upload and the three launches on `stream`; the equalised image goes to dst and, when not NULL, to dst2 (W x H bytes, rows W apart)
static int enqueue(vclahe_ctx* c, hipStream_t stream, const uint8_t* gray, const int row_stride, uint8_t* dst, uint8_t* dst2) {
    const vilclahe_stage::Staged s = vilclahe_stage::stage_image(c, gray, row_stride);
    VILCHK(hipMemcpyAsync(s.dev, s.host, (size_t)c->cfg.width * c->cfg.height, hipMemcpyHostToDevice, stream));
    return vilclahe_stage::enqueue_kernels(c, stream, dst, dst2);
}

static void account(vclahe_ctx* c, uint8_t* out, const int out_stride) {
    for (int k = 0; k < VCLAHE_NUM_KERNELS; ++k) c->prof.span(k, k, k + 1);
    c->ran = true;
    if (out) for (int y = 0; y < c->cfg.height; ++y) memcpy(out + (size_t)y * out_stride, c->h_out + (size_t)y * c->cfg.width, c->cfg.width);
}

extern "C" {

int vclahe_create(int32_t device, const vclahe_cfg* cfg, vclahe_ctx** out) {
    if (!out || !cfg || cfg->width < 16 || cfg->width > 16384 || cfg->height < 16 || cfg->height > 16384 || cfg->tiles_x < 1 || cfg->tiles_x > VCLAHE_MAX_TILES ||
        cfg->tiles_y < 1 || cfg->tiles_y > VCLAHE_MAX_TILES || !std::isfinite(cfg->clip_limit) || cfg->clip_limit < 0.0)
        return VIL_ERR_INVALID_ARGUMENT;
    vclahe_ctx* c = new vclahe_ctx();
    c->cfg = *cfg;
    const int W = cfg->width, H = cfg->height;
    int We = W, He = H;                                                                             // step 1
    if (W % cfg->tiles_x || H % cfg->tiles_y) { We = W + cfg->tiles_x - W % cfg->tiles_x; He = H + cfg->tiles_y - H % cfg->tiles_y; }
    c->tw = We / cfg->tiles_x; c->th = He / cfg->tiles_y;
    const int area = c->tw * c->th;                                                                 // <= 16400^2 < 2^29
    if (cfg->clip_limit > 0.0) {                                                                    // step 2
        const double v = cfg->clip_limit * area / 256;
        c->clip = v >= (double)area ? area : std::max((int)v, 1);
    }
    c->lut_scale = 255.0f / (float)area; c->inv_tw = 1.0f / (float)c->tw; c->inv_th = 1.0f / (float)c->th;
    c->shares = std::min((area + VC_SHARE - 1) / VC_SHARE, VC_MAX_SHARES);
    c->chunk = (area + c->shares - 1) / c->shares;                                                  // shares * chunk < area + shares
    const size_t WH = (size_t)W * H, T = (size_t)cfg->tiles_x * cfg->tiles_y;
    vilhost::Arena a;
    c->o_hist = a.take(T * 1024); c->o_lut = a.take(T * 256); c->o_src = a.take(WH); c->o_out = a.take(WH);
    hipError_t err = c->open(device, a.bytes);
    if (err == hipSuccess) err = c->pin(&c->h_img, vilhost::up16(WH));
    if (err == hipSuccess) err = c->pin(&c->h_out, vilhost::up16(WH));
    if (err == hipSuccess) err = hipMemsetAsync(c->d_mem, 0, a.bytes, c->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(c->stream);
    if (err != hipSuccess) { vclahe_destroy(c); VILCHK(err); }
    *out = c;
    return VIL_OK;
}

void vclahe_destroy(vclahe_ctx* c) {
    if (!c) return;
    c->close(c->prof);
    delete c;
}

int vclahe_profile_enable(vclahe_ctx* c, int32_t enable) {
    if (!c) return VIL_ERR_INVALID_ARGUMENT;
    VILCHK(c->prof.enable(c->device, enable != 0));
    return VIL_OK;
}
int vclahe_profile_read(vclahe_ctx* c, int64_t* launches3, double* total_ms3) {
    if (!c || !launches3 || !total_ms3) return VIL_ERR_INVALID_ARGUMENT;
    c->prof.read(launches3, total_ms3);
    return VIL_OK;
}

int vclahe_apply(vclahe_ctx* c, const uint8_t* gray, int32_t row_stride, uint8_t* out, int32_t out_stride) {
    if (!c || !gray || !out || row_stride < c->cfg.width || out_stride < c->cfg.width) return VIL_ERR_INVALID_ARGUMENT;
    VILCHK(hipSetDevice(c->device));
    uint8_t* d_out = (uint8_t*)(c->d_mem + c->o_out);
    const int st = enqueue(c, c->stream, gray, row_stride, d_out, nullptr);
    if (st != VIL_OK) return st;
    VILCHK(hipMemcpyAsync(c->h_out, d_out, (size_t)c->cfg.width * c->cfg.height, hipMemcpyDeviceToHost, c->stream));
    VILCHK(hipStreamSynchronize(c->stream));
    VILCHK(hipGetLastError());
    account(c, out, out_stride);
    return VIL_OK;
}

int vclahe_push(vclahe_ctx* c, vtrack_ctx* tracker, const uint8_t* gray, int32_t row_stride, uint8_t* out, int32_t out_stride) {
    if (!c || !tracker || !gray || row_stride < c->cfg.width || (out && out_stride < c->cfg.width)) return VIL_ERR_INVALID_ARGUMENT;
    const viltrack_stage::Target tg = viltrack_stage::target(tracker);
    if (tg.width != c->cfg.width || tg.height != c->cfg.height || tg.device != c->device) return VIL_ERR_INVALID_ARGUMENT;
    VILCHK(hipSetDevice(c->device));
    uint8_t* d_out = (uint8_t*)(c->d_mem + c->o_out);
    int st = enqueue(c, tg.stream, gray, row_stride, tg.level0, out ? d_out : nullptr);             // stage 1 of the tracker's push
    if (st != VIL_OK) return st;
    if (out) VILCHK(hipMemcpyAsync(c->h_out, d_out, (size_t)c->cfg.width * c->cfg.height, hipMemcpyDeviceToHost, tg.stream));
    st = viltrack_stage::finish_push(tracker);                                                      // stage 2: pyramid, the synchronisation, the flip
    if (st != VIL_OK) return st;
    account(c, out, out_stride);
    return VIL_OK;
}

int vclahe_debug_read(vclahe_ctx* c, int32_t what, void* dst, int64_t capacity_bytes) {
    if (!c || !dst || !c->ran) return VIL_ERR_INVALID_ARGUMENT;
    const size_t T = (size_t)c->cfg.tiles_x * c->cfg.tiles_y;
    size_t off = 0, bytes = 0;
    switch (what) {
    case VCLAHE_DBG_HIST: off = c->o_hist; bytes = T * 1024; break;
    case VCLAHE_DBG_LUT: off = c->o_lut; bytes = T * 256; break;
    default: return VIL_ERR_INVALID_ARGUMENT;
    }
    if (capacity_bytes < (int64_t)bytes) return VIL_ERR_INVALID_ARGUMENT;
    VILCHK(hipSetDevice(c->device));
    VILCHK(hipMemcpyAsync(dst, c->d_mem + off, bytes, hipMemcpyDeviceToHost, c->stream));
    VILCHK(hipStreamSynchronize(c->stream));
    return VIL_OK;
}

}  // extern "C"
