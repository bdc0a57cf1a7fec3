// vildepth.hip -- LiDAR depth association of visual features on gfx950 behind include/vildepth.h
// (feature_tracker_/src/feature_tracker.h: DepthRegister::get_depth :98-343; the steps are numbered as in the header).
//
// The world-frame depth cloud is resident (vdepth_set_cloud).  One vdepth_register is one submission: the matrices and the features go up,
// the range image (VDEPTH_BINS^2 x 8 B) and the counters are cleared on the stream, then
//   k_depth_project  a thread per cloud point: steps 1-4.  The bin's winner is ONE 64-bit atomicMin on (dist bits << 32 | cloud index):
//                    dist > 0 orders like its bit pattern and the index breaks ties towards the earlier point, so the image does not depend
//                    on the order the atomics arrive in.  The thread that finds its bin empty also counts the bin in its row's counter.
//   k_depth_compact  a workgroup per image row: the rows above it summed from the row counters (its entry of the 361-entry row table), its
//                    own occupied bins ranked by ballot + popcount prefix -- a stable partition without atomics, the emission order is part
//                    of the contract --, the winner's point transformed again with the instructions of k_depth_project, [x/r y/r z/r r] out.
//   k_depth_query    a wave per feature: steps 7-9.  EXACT 3-NN over the sphere points whose image row is within VD_BAND rows of the
//                    feature's own row: an accepted neighbour is less than 2.5003 degrees away, so at most 6 rows;
//                    row-major emission makes the candidates one contiguous slice of the sphere cloud, read as coalesced 16-byte loads.  A
//                    lane keeps its three best (distance bits << 32 | index) keys, the wave merges them with three 64-bit min reductions.
// The float arithmetic of the reference is kept unfused and in source order (x86 g++ and numpy do not contract a * b + c; hipcc would):
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/vildepth.h"
#include "vil_host.hpp"
#include "vil_knn.hpp"
#include "vil_math.hpp"
#include "vildepth_stage.hpp"

#define VD_BINS VDEPTH_BINS
#define VD_IMG (VD_BINS * VD_BINS)
#define VD_BAND 7
#define VD_ROW_THREADS 384           // >= VD_BINS, whole waves
#define VD_ROW_WAVES (VD_ROW_THREADS / 64)
#define VD_EMPTY (~0ull)
#define VD_TAB 368                   // ints reserved for a VD_BINS(+1)-entry table

namespace {

// counters of one call (ints), read back in front of the depths
enum { H_INVIEW = 0, H_NSPHERE, H_WITH, H_INTS = 16 };

// step 1: both transforms of a cloud point; false when a coordinate is not finite after either.  M: world_to_lidar, then lidar_to_view
__device__ __forceinline__ bool view_point(const float4 w, const float* __restrict__ M, float& x, float& y, float& z) {
    const float ax = ((M[0] * w.x + M[1] * w.y) + M[2] * w.z) + M[3];
    const float ay = ((M[4] * w.x + M[5] * w.y) + M[6] * w.z) + M[7];
    const float az = ((M[8] * w.x + M[9] * w.y) + M[10] * w.z) + M[11];
    if (!(isfinite(ax) && isfinite(ay) && isfinite(az))) return false;
    x = ((M[12] * ax + M[13] * ay) + M[14] * az) + M[15];
    y = ((M[16] * ax + M[17] * ay) + M[18] * az) + M[19];
    z = ((M[20] * ax + M[21] * ay) + M[22] * az) + M[23];
    return isfinite(x) && isfinite(y) && isfinite(z);
}
__device__ __forceinline__ float range_of(const float x, const float y, const float z) { return sqrtf(x * x + y * y + z * z); }
// step 3, the row: finite inputs give a row angle in [0, 180] and a row in [0, VD_BINS]
__device__ __forceinline__ int row_of(const float x, const float y, const float z) {
    const float row_angle = (float)((double)atan2f(z, sqrtf(x * x + y * y)) * 180.0 / M_PI + 90.0);
    return (int)roundf(row_angle / 0.5f);
}
__device__ __forceinline__ int col_of(const float x, const float y) {
    const float col_angle = (float)((double)atan2f(x, y) * 180.0 / M_PI);
    return (int)roundf(col_angle / 0.5f);
}

__global__ __launch_bounds__(256) void k_depth_project(int n, const float4* __restrict__ cloud, const float* __restrict__ M, unsigned long long* __restrict__ img,
                                                       int* __restrict__ rowcnt, int* __restrict__ hdr) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float x, y, z;
    if (!view_point(cloud[i], M, x, y, z)) return;
    if (x < 0.0f || fabsf(y / x) > 10.0f || fabsf(z / x) > 10.0f) return;                          // step 2
    const int row = row_of(x, y, z), col = col_of(x, y);
    if (row < 0 || row >= VD_BINS || col < 0 || col >= VD_BINS) return;
    const float dist = range_of(x, y, z);
    if (!(dist > 0.0f && dist < FLT_MAX)) return;
    const unsigned long long key = ((unsigned long long)__float_as_uint(dist) << 32) | (unsigned)i;
    const unsigned long long old = atomicMin(&img[row * VD_BINS + col], key);                      // row, col in [0, VD_BINS): inside the image
    if (old == VD_EMPTY) atomicAdd(&rowcnt[row], 1);                                                // exactly one thread per occupied bin sees it empty
    atomicAdd(&hdr[H_INVIEW], 1);
}

__global__ __launch_bounds__(VD_ROW_THREADS) void k_depth_compact(const float4* __restrict__ cloud, const float* __restrict__ M, const unsigned long long* __restrict__ img,
                                                                  const int* __restrict__ rowcnt, int* __restrict__ rowtab, float4* __restrict__ sphere, int* __restrict__ hdr) {
    __shared__ int s_lo[VD_ROW_WAVES], s_w[VD_ROW_WAVES];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = blockIdx.x;
    int lo = t < r ? rowcnt[t] : 0;                                                                 // r <= VD_BINS - 1 < VD_ROW_THREADS
    for (int o = 32; o; o >>= 1) lo += __shfl_xor(lo, o);
    const unsigned long long key = t < VD_BINS ? img[r * VD_BINS + t] : VD_EMPTY;
    const bool occ = key != VD_EMPTY;
    const unsigned long long b = __ballot(occ);
    if (lane == 0) { s_lo[wave] = lo; s_w[wave] = __popcll(b); }
    __syncthreads();
    int start = 0, off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < VD_ROW_WAVES; ++w) { start += s_lo[w]; const int c = s_w[w]; off += w < wave ? c : 0; tot += c; }
    if (t == 0) {
        rowtab[r] = start;
        if (r == VD_BINS - 1) { rowtab[VD_BINS] = start + tot; hdr[H_NSPHERE] = start + tot; }
    }
    const int pos = start + off + __popcll(b & ((1ull << lane) - 1ull));
    if (occ && pos < VD_IMG) {                                                                      // pos < occupied bins <= VD_IMG by construction
        float x = 0.f, y = 0.f, z = 0.f;
        view_point(cloud[(unsigned)key], M, x, y, z);                                               // the index was written by a thread with i < n
        const float range = range_of(x, y, z);                                                      // step 6: the bits of key >> 32
        sphere[pos] = make_float4(x / range, y / range, z / range, range);
    }
}

__global__ __launch_bounds__(256) void k_depth_query(int n_feat, const float* __restrict__ feat, const float4* __restrict__ sphere, const int* __restrict__ rowtab, float thr,
                                                     float* __restrict__ depth, int* __restrict__ nn3, int* __restrict__ hdr) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n_feat) return;                                                                        // wave-uniform
    const int ns = rowtab[VD_BINS];
    const float fx = feat[3 * i], fy = feat[3 * i + 1], fz = feat[3 * i + 2];
    const float nrm = sqrtf((fx * fx + fy * fy) + fz * fz);                                         // step 7
    const float px = fz / nrm, py = -(fx / nrm), pz = -(fy / nrm);
    float out = -1.0f;
    int i0 = -1, i1 = -1, i2 = -1;
    if (ns >= VDEPTH_MIN_SPHERE && isfinite(px) && isfinite(py) && isfinite(pz)) {
        const int row = row_of(px, py, pz), lo = max(row - VD_BAND, 0), hi = min(row + VD_BAND, VD_BINS - 1);
        unsigned long long k0 = VD_EMPTY, k1 = VD_EMPTY, k2 = VD_EMPTY;
        if (lo <= hi) {
            const int e = min(rowtab[hi + 1], ns);
            for (int j = rowtab[lo] + lane; j < e; j += 64) {                                       // 0 <= rowtab[lo], j < ns: inside the sphere cloud
                const float4 q = sphere[j];
                const unsigned long long key = ((unsigned long long)__float_as_uint(vknn::sqdist_nofma(px, py, pz, q.x, q.y, q.z)) << 32) | (unsigned)j;
                if (key < k2) {
                    if (key < k1) { k2 = k1; if (key < k0) { k1 = k0; k0 = key; } else k1 = key; }
                    else k2 = key;
                }
            }
        }
        unsigned long long best[3];
#pragma unroll
        for (int t = 0; t < 3; ++t) {                                                               // a key is unique (its index): one lane pops
            best[t] = vd::wave_min64(k0);
            if (k0 == best[t] && k0 != VD_EMPTY) { k0 = k1; k1 = k2; k2 = VD_EMPTY; }
        }
        if (best[2] != VD_EMPTY && __uint_as_float((unsigned)(best[2] >> 32)) < thr) {             // step 8
            i0 = (int)(unsigned)best[0]; i1 = (int)(unsigned)best[1]; i2 = (int)(unsigned)best[2];
            const float r1 = sphere[i0].w, r2 = sphere[i1].w, r3 = sphere[i2].w;                    // step 9
            const float mn = fminf(r1, fminf(r2, r3)), mx = fmaxf(r1, fmaxf(r2, r3));
            if (!(mx - mn > 2.0f)) {
                const float s = ((r1 + r2) + r3) / 3.0f;
                const float d = px * s;
                if (d > 3.0f) out = d;
            }
        }
    }
    if (lane == 0) {
        depth[i] = out; nn3[3 * i] = i0; nn3[3 * i + 1] = i1; nn3[3 * i + 2] = i2;
        if (out != -1.0f) atomicAdd(&hdr[H_WITH], 1);
    }
}

}  // namespace

struct vdepth_ctx : vilhost::Device {        // d_mem: cloud | image | row counters, counters, depths | row table | sphere | matrices, features | nn3
    int max_cloud = 0, max_feat = 0, n_cloud = 0;
    float thr = 0.f;                                        // step 8's threshold
    char* h_cloud = nullptr; char* h_in = nullptr; char* h_out = nullptr;      // pinned: cloud upload, matrices + features, counters + depths
    size_t o_cloud = 0, o_img = 0, o_rowcnt = 0, o_hdr = 0, o_depth = 0, o_rowtab = 0, o_sphere = 0, o_in = 0, o_nn3 = 0;
    int last_sphere = 0, last_feat = 0; bool last_on_device = false;          // what vdepth_debug_read reads
    vilhost::Profiler<VDEPTH_NUM_KERNELS, VDEPTH_NUM_KERNELS + 1> prof;
};

// ---- the hand-over stage (vildepth_stage.hpp) --------------------------------------------------------------------------------------
vildepth_stage::Target vildepth_stage::target(const vdepth_ctx* c) { return {c->device, c->max_cloud}; }
int vildepth_stage::replace_cloud(vdepth_ctx* c, const int n, const float* src, const hipMemcpyKind kind) {
    if (n) {
        VILCHK(hipSetDevice(c->device));
        VILCHK(hipMemcpyAsync(c->d_mem + c->o_cloud, src, 16 * (size_t)n, kind, c->stream));
        VILCHK(hipStreamSynchronize(c->stream));
    }
    c->n_cloud = n;
    return VIL_OK;
}

extern "C" {

int vdepth_create(int32_t device, int32_t max_cloud_points, int32_t max_features, vdepth_ctx** out) {
    if (!out || max_cloud_points < 1 || max_features < 1) return VIL_ERR_INVALID_ARGUMENT;
    vdepth_ctx* c = new vdepth_ctx();
    c->max_cloud = max_cloud_points; c->max_feat = max_features;
    c->thr = (float)std::pow(std::sin(0.5 / 180.0 * M_PI) * 5.0, 2);
    const size_t N = (size_t)max_cloud_points, F = (size_t)max_features;
    static_assert((4 * VD_TAB) % 16 == 0 && (4 * H_INTS) % 16 == 0, "the three fields below must lie back to back");
    vilhost::Arena a;
    c->o_cloud = a.take(16 * N);
    c->o_img = a.take(8 * (size_t)VD_IMG);
    c->o_rowcnt = a.take(4 * VD_TAB);                       // row counters and counters are cleared together,
    c->o_hdr = a.take(4 * H_INTS);                          // counters and depths are read back together
    c->o_depth = a.take(4 * F);
    c->o_rowtab = a.take(4 * VD_TAB);
    c->o_sphere = a.take(16 * (size_t)VD_IMG);
    c->o_in = a.take(4 * (24 + 3 * F));
    c->o_nn3 = a.take(12 * F);
    hipError_t err = c->open(device, a.bytes);
    if (err == hipSuccess) err = c->pin(&c->h_cloud, 16 * N);
    if (err == hipSuccess) err = c->pin(&c->h_in, vilhost::up16(4 * (24 + 3 * F)));
    if (err == hipSuccess) err = c->pin(&c->h_out, 4 * H_INTS + vilhost::up16(4 * F));
    if (err != hipSuccess) { vdepth_destroy(c); VILCHK(err); }
    *out = c;
    return VIL_OK;
}

void vdepth_destroy(vdepth_ctx* c) {
    if (!c) return;
    c->close(c->prof);
    delete c;
}

int vdepth_profile_enable(vdepth_ctx* c, int32_t enable) {
    if (!c) return VIL_ERR_INVALID_ARGUMENT;
    VILCHK(c->prof.enable(c->device, enable != 0));
    return VIL_OK;
}
int vdepth_profile_read(vdepth_ctx* c, int64_t* launches3, double* total_ms3) {
    if (!c || !launches3 || !total_ms3) return VIL_ERR_INVALID_ARGUMENT;
    c->prof.read(launches3, total_ms3);
    return VIL_OK;
}

int vdepth_set_cloud(vdepth_ctx* c, int32_t n, const float* xyzi) {
    if (!c || n < 0 || n > c->max_cloud || (n && !xyzi)) return VIL_ERR_INVALID_ARGUMENT;
    if (n) memcpy(c->h_cloud, xyzi, 16 * (size_t)n);
    return vildepth_stage::replace_cloud(c, n, (const float*)c->h_cloud, hipMemcpyHostToDevice);
}

int vdepth_register(vdepth_ctx* c, const float* world_to_lidar, const float* lidar_to_view, int32_t n_feat, const float* feat_xyz, float* depth_out, vdepth_summary* out) {
    if (!c || !world_to_lidar || !lidar_to_view || n_feat < 0 || n_feat > c->max_feat || (n_feat && (!feat_xyz || !depth_out))) return VIL_ERR_INVALID_ARGUMENT;
    const int n = c->n_cloud;
    int* hdr = (int*)c->h_out;
    c->last_feat = n_feat; c->last_sphere = 0; c->last_on_device = false;
    if (n == 0) {                                           // :109: no cloud, nothing to submit
        memset(hdr, 0, 4 * H_INTS);
        for (int i = 0; i < n_feat; ++i) depth_out[i] = -1.0f;
    } else {
        VILCHK(hipSetDevice(c->device));
        float* in = (float*)c->h_in;
        memcpy(in, world_to_lidar, 48); memcpy(in + 12, lidar_to_view, 48);
        if (n_feat) memcpy(in + 24, feat_xyz, 12 * (size_t)n_feat);
        char* d = c->d_mem;
        const float4* d_cloud = (const float4*)(d + c->o_cloud); unsigned long long* d_img = (unsigned long long*)(d + c->o_img);
        int* d_rowcnt = (int*)(d + c->o_rowcnt); int* d_hdr = (int*)(d + c->o_hdr); int* d_rowtab = (int*)(d + c->o_rowtab);
        float4* d_sphere = (float4*)(d + c->o_sphere); const float* d_in = (const float*)(d + c->o_in);
        VILCHK(hipMemcpyAsync(d + c->o_in, in, 4 * (24 + 3 * (size_t)n_feat), hipMemcpyHostToDevice, c->stream));
        VILCHK(hipMemsetAsync(d_img, 0xff, 8 * (size_t)VD_IMG, c->stream));
        VILCHK(hipMemsetAsync(d_rowcnt, 0, 4 * (VD_TAB + H_INTS), c->stream));
        VILCHK(c->prof.mark(0, c->stream));
        hipLaunchKernelGGL(k_depth_project, dim3((n + 255) / 256), dim3(256), 0, c->stream, n, d_cloud, d_in, d_img, d_rowcnt, d_hdr);
        VILCHK(c->prof.mark(1, c->stream));
        hipLaunchKernelGGL(k_depth_compact, dim3(VD_BINS), dim3(VD_ROW_THREADS), 0, c->stream, d_cloud, d_in, d_img, d_rowcnt, d_rowtab, d_sphere, d_hdr);
        VILCHK(c->prof.mark(2, c->stream));
        if (n_feat) hipLaunchKernelGGL(k_depth_query, dim3((n_feat + 3) / 4), dim3(256), 0, c->stream, n_feat, d_in + 24, d_sphere, d_rowtab, c->thr, (float*)(d + c->o_depth),
                                       (int*)(d + c->o_nn3), d_hdr);
        VILCHK(c->prof.mark(3, c->stream));
        VILCHK(hipMemcpyAsync(c->h_out, d_hdr, 4 * H_INTS + 4 * (size_t)n_feat, hipMemcpyDeviceToHost, c->stream));
        VILCHK(hipStreamSynchronize(c->stream));
        VILCHK(hipGetLastError());
        for (int k = 0; k < (n_feat ? 3 : 2); ++k) c->prof.span(k, k, k + 1);                       // no features: k_depth_query was not launched
        if (n_feat) memcpy(depth_out, c->h_out + 4 * H_INTS, 4 * (size_t)n_feat);
        c->last_sphere = hdr[H_NSPHERE]; c->last_on_device = true;
    }
    if (out) { out->n_cloud = n; out->n_in_view = hdr[H_INVIEW]; out->n_sphere = hdr[H_NSPHERE]; out->n_with_depth = hdr[H_WITH]; }
    return VIL_OK;
}

int vdepth_debug_read(vdepth_ctx* c, float* sphere_xyzr, int32_t capacity, int32_t* nn3) {
    if (!c || (sphere_xyzr && capacity < c->last_sphere)) return VIL_ERR_INVALID_ARGUMENT;
    if (!c->last_on_device) {
        if (nn3) for (int i = 0; i < 3 * c->last_feat; ++i) nn3[i] = -1;
        return VIL_OK;
    }
    VILCHK(hipSetDevice(c->device));
    if (sphere_xyzr && c->last_sphere) VILCHK(hipMemcpyAsync(sphere_xyzr, c->d_mem + c->o_sphere, 16 * (size_t)c->last_sphere, hipMemcpyDeviceToHost, c->stream));
    if (nn3 && c->last_feat) VILCHK(hipMemcpyAsync(nn3, c->d_mem + c->o_nn3, 12 * (size_t)c->last_feat, hipMemcpyDeviceToHost, c->stream));
    VILCHK(hipStreamSynchronize(c->stream));
    return VIL_OK;
}

}  // extern "C"
