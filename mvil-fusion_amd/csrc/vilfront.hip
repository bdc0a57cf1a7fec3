// vilfront.hip -- the scan-to-scan LiDAR front end as one resident call on gfx950, behind include/vilfront.h (Estimator::processLidar,
// estimator.cpp:122-436; the de-skew's steps are numbered as in the header).
//
// New here is the de-skew and what hands its result on; everything else is the other rows' code, called through their hidden stages:
//   k_front_deskew   a thread per raw point: steps 0-8 and the keep flag of steps 3 and 9; the workgroup's number of kept points.
//   k_front_scan     ONE workgroup: the exclusive sum of the workgroups' counts in place, and the total (n_kept).
//   k_front_scatter  a thread per raw point: its rank among its workgroup's kept points (a ballot per wave, the waves' counts through
//                    LDS) behind the workgroup's offset -- the survivors keep their input order.
//   (filter A)       vilcloud_stage::filter_resident on the private vcloud_ctx's stream, between two events.
//   k_front_xyz      a thread per centroid: [x y z intensity] -> the stride-3 cloud the registration and the fitness search read; the
//                    non-finite flag.
// No atomics, no workgroup waits for another.  Every point count a kernel needs is read from the header on the device; grids are sized
// from the number of raw points.  After the one wait that brings the header back the host knows n_filtered and drives the exchange of
// the resident pair: vgicp_promote_source, villoop_stage::promote_source, the two install_source stages, vgicp_align, vloop_score.
// The float arithmetic of the contract is kept unfused and in source order (hipcc would contract a * b + c):
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/vilfront.h"
#include "vil_host.hpp"
#include "vilcloud_stage.hpp"
#include "villoop_stage.hpp"
#include "vilvgicp_stage.hpp"

#define VF_BLK 256
#define VF_WAVES (VF_BLK / 64)
#define VF_MAX_POINTS (1 << 27)

namespace {

enum { K_DESKEW = 0, K_SCAN, K_SCATTER, K_XYZ };
static_assert(K_XYZ + 1 == VFRONT_NUM_KERNELS, "one profile entry per kernel");
// the device header (ints)
enum { H_KEPT = 0, H_FILT, H_NONFINITE, H_INTS = 16 };

struct Motion { float qw, qx, qy, qz, tx, ty, tz, time_factor; };

// step 7: Eigen's quaternion * vector
__device__ __forceinline__ void rotate(const float qw, const float qx, const float qy, const float qz, float& x, float& y, float& z) {
    float ax = qy * z - qz * y, ay = qz * x - qx * z, az = qx * y - qy * x;
    ax = ax + ax; ay = ay + ay; az = az + az;
    const float bx = qy * az - qz * ay, by = qz * ax - qx * az, bz = qx * ay - qy * ax;
    x = (x + qw * ax) + bx; y = (y + qw * ay) + by; z = (z + qw * az) + bz;
}

// steps 0-9 for one point; false: rejected or removed
__device__ __forceinline__ bool deskew_point(const float4 p, const Motion m, const double dmin, const double dmax, float4& out) {
    if (!(p.w >= -2147483648.0f && p.w < 2147483648.0f)) return false;                              // step 0 (false for NaN)
    const float whole = (float)(int)p.w;
    const float distance = sqrtf(p.x * p.x + p.y * p.y);                                            // step 1
    const float s = m.time_factor * (p.w - whole);                                                  // step 2
    if (s < 0.0f || (double)s > 1.001 || (double)distance < dmin || (double)distance > dmax) return false;      // step 3
    float x = p.x - s * m.tx, y = p.y - s * m.ty, z = p.z - s * m.tz;                                // step 4
    const float d = m.qw, absD = fabsf(d);                                                          // step 5
    float scale0, scale1;
    if (absD >= 1.0f - FLT_EPSILON) { scale0 = 1.0f - s; scale1 = s; }
    else {
        const float theta = acosf(absD), sinTheta = sinf(theta);
        scale0 = sinf((1.0f - s) * theta) / sinTheta;
        scale1 = sinf(s * theta) / sinTheta;
    }
    if (d < 0.0f) scale1 = -scale1;
    float cw = scale0 + scale1 * m.qw, cx = -(scale1 * m.qx), cy = -(scale1 * m.qy), cz = -(scale1 * m.qz);      // step 6
    const float n2 = ((cx * cx + cy * cy) + cz * cz) + cw * cw;
    if (n2 > 0.0f) { const float nrm = sqrtf(n2); cw = cw / nrm; cx = cx / nrm; cy = cy / nrm; cz = cz / nrm; }
    rotate(cw, cx, cy, cz, x, y, z);                                                                // step 7
    rotate(m.qw, m.qx, m.qy, m.qz, x, y, z);
    x = x + m.tx; y = y + m.ty; z = z + m.tz;                                                       // step 8
    out = make_float4(x, y, z, whole);
    return isfinite(x) && isfinite(y) && isfinite(z);                                               // step 9
}

// tmp[i], flag[i] for i < n; bcount[blockIdx.x] (the grid has ceil(max(n, 1) / VF_BLK) workgroups, bcount one entry per workgroup)
__global__ __launch_bounds__(VF_BLK) void k_front_deskew(int n, const float4* __restrict__ in, Motion m, double dmin, double dmax, float4* __restrict__ tmp, int* __restrict__ flag,
                                                         int* __restrict__ bcount) {
    const int i = blockIdx.x * VF_BLK + threadIdx.x;
    bool keep = false;
    if (i < n) {
        float4 out = make_float4(0.f, 0.f, 0.f, 0.f);
        keep = deskew_point(in[i], m, dmin, dmax, out);
        tmp[i] = out; flag[i] = keep ? 1 : 0;
    }
    const int cnt = __syncthreads_count(keep ? 1 : 0);
    if (threadIdx.x == 0) bcount[blockIdx.x] = cnt;
}

// bcount[0 .. nblk) becomes its exclusive prefix sum, *total the sum.  ONE workgroup, VF_BLK entries per round with a carry.
__global__ __launch_bounds__(VF_BLK) void k_front_scan(int nblk, int* __restrict__ bcount, int* __restrict__ total) {
    __shared__ int s_w[VF_WAVES];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int carry = 0;
    for (int b0 = 0; b0 < nblk; b0 += VF_BLK) {
        const int v = b0 + t < nblk ? bcount[b0 + t] : 0;
        int inc = v;
        for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(inc, o); if (lane >= o) inc += u; }
        if (lane == 63) s_w[wave] = inc;
        __syncthreads();
        int before = 0, all = 0;
        for (int w = 0; w < VF_WAVES; ++w) { const int c = s_w[w]; before += w < wave ? c : 0; all += c; }
        if (b0 + t < nblk) bcount[b0 + t] = carry + before + inc - v;
        carry += all;
        __syncthreads();
    }
    if (t == 0) *total = carry;
}

// the kept points, in input order: boff[blockIdx.x] + the rank in the workgroup < n_kept <= n, inside `out`
__global__ __launch_bounds__(VF_BLK) void k_front_scatter(int n, const float4* __restrict__ tmp, const int* __restrict__ flag, const int* __restrict__ boff, float4* __restrict__ out) {
    __shared__ int s_w[VF_WAVES];
    const int i = blockIdx.x * VF_BLK + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool keep = i < n && flag[i] != 0;
    const unsigned long long b = __ballot(keep);
    if (lane == 0) s_w[wave] = __popcll(b);
    __syncthreads();
    int before = 0;
    for (int w = 0; w < VF_WAVES; ++w) before += w < wave ? s_w[w] : 0;
    if (keep) out[boff[blockIdx.x] + before + __popcll(b & ((1ull << lane) - 1ull))] = tmp[i];
}

// the filtered cloud as float xyz, stride 3; hdr[H_NONFINITE] (cleared at the start of the call) is set by every thread that finds one
__global__ __launch_bounds__(VF_BLK) void k_front_xyz(int* __restrict__ hdr, int n_upper, const float4* __restrict__ f, float* __restrict__ xyz) {
    const int k = blockIdx.x * VF_BLK + threadIdx.x;
    if (k >= min(hdr[H_FILT], n_upper)) return;
    const float4 p = f[k];
    xyz[3 * (size_t)k] = p.x; xyz[3 * (size_t)k + 1] = p.y; xyz[3 * (size_t)k + 2] = p.z;
    if (!(isfinite(p.x) && isfinite(p.y) && isfinite(p.z))) hdr[H_NONFINITE] = 1;
}

bool finite_all(const double* v, int n) { for (int k = 0; k < n; ++k) if (!std::isfinite(v[k])) return false; return true; }

}  // namespace

struct vfront_ctx : vilhost::Device {        // d_mem: header | raw scan | de-skewed, uncompacted | flags | workgroup counts | de-skewed | filtered | filtered xyz
    int msp = 0;                                            // max_scan_points
    vcloud_ctx* cloud = nullptr; vgicp_ctx* reg = nullptr; vloop_ctx* loop = nullptr;      // private, through the public constructors
    char* h_io = nullptr; int* h_hdr = nullptr;             // pinned: points in either direction; the header
    size_t o_hdr = 0, o_raw = 0, o_tmp = 0, o_flag = 0, o_bcount = 0, o_kept = 0, o_filt = 0, o_xyz = 0;
    vilhost::Fence ready, done;                             // around the filter, which runs on the vcloud_ctx's stream
    bool has_prev = false, broken = false;
    int last_kept = 0, last_filt = 0;                       // what vfront_read_deskewed and vfront_debug_read read
    vilhost::EventLog<VFRONT_NUM_KERNELS> prof;

    template <class T> T* at(size_t o) { return (T*)(d_mem + o); }
};

namespace {

int read_points(vfront_ctx* c, const size_t offset, const int n_have, float* out, const int32_t capacity, int32_t* n) {
    if (!n) return VIL_ERR_INVALID_ARGUMENT;
    *n = n_have;
    if (capacity < n_have || (n_have && !out)) return VIL_ERR_INVALID_ARGUMENT;
    if (n_have) {
        VILCHK(hipSetDevice(c->device));
        VILCHK(hipMemcpyAsync(c->h_io, c->d_mem + offset, 16 * (size_t)n_have, hipMemcpyDeviceToHost, c->stream));
        VILCHK(hipStreamSynchronize(c->stream));
        memcpy(out, c->h_io, 16 * (size_t)n_have);
    }
    return VIL_OK;
}

bool options_ok(const vfront_options& o) {
    const double d[4] = {o.lidar_time_step, o.min_distance, o.max_distance, o.resolution};
    const double r[3] = {o.reg.rotation_epsilon, o.reg.transformation_epsilon, o.reg.lm_init_lambda_factor};
    if (!finite_all(d, 4) || !finite_all(r, 3) || !(o.lidar_time_step > 0.0) || !(o.resolution > 0.0)) return false;
    if (!std::isfinite((float)(1.0 / o.lidar_time_step))) return false;
    return vilcloud_stage::accepts(o.leaf, o.hist_size) && vilvgicp_stage::accepts(o.reg);
}

// steps 3-6 of vfront_push_scan, after the wait that told the host n_filt >= 1.  VIL_ERR_DEVICE from here breaks the context.
int exchange_and_align(vfront_ctx* c, const int n_filt, const double* guess, const vfront_options& o, vfront_summary& s) {
    const float* d_xyz = c->at<float>(c->o_xyz);
    int st;
    if (c->has_prev) {                                                                              // step 3, before step 4 overwrites the sources
        if ((st = vgicp_promote_source(c->reg, o.resolution)) != VIL_OK) return st;
        if ((st = villoop_stage::promote_source(c->loop)) != VIL_OK) return st;
    }
    // step 4: d_xyz was written on this context's stream, which the host has waited for
    if ((st = vilvgicp_stage::install_source(c->reg, n_filt, d_xyz, nullptr, hipMemcpyDeviceToDevice)) != VIL_OK) return st;
    if ((st = villoop_stage::install_source(c->loop, n_filt, d_xyz, hipMemcpyDeviceToDevice)) != VIL_OK) return st;
    const bool had_prev = c->has_prev;
    c->has_prev = true;                                                                             // step 6: all_lidar_frame holds the scan before it is aligned (:250)
    s.accepted = 1;
    if (!had_prev) return VIL_OK;
    double g[16], T[16];                                                                            // step 5
    for (int q = 0; q < 16; ++q) g[q] = guess ? (double)(float)guess[q] : (q % 5 == 0 ? 1.0 : 0.0);  // Matrix<float, 4, 4> guss, :291
    vgicp_summary sm;
    if ((st = vgicp_align(c->reg, g, &o.reg, T, &sm)) != VIL_OK) return st;
    for (int q = 0; q < 16; ++q) T[q] = (double)(float)T[q];                                        // getFinalTransformation() is a Matrix4f, :313
    double score = 0.0; int32_t used = 0;
    if ((st = vloop_score(c->loop, 1, T, DBL_MAX, &score, &used, nullptr, nullptr)) != VIL_OK) return st;
    s.aligned = 1; s.n_used = used; s.fitness = score; s.reg = sm;
    memcpy(s.T, T, sizeof T);
    return VIL_OK;
}

}  // namespace

extern "C" {

void vfront_default_options(vfront_options* o) {
    if (!o) return;
    o->deskew = 1; o->hist_size = 512; o->lidar_time_step = 0.1; o->min_distance = 0.5; o->max_distance = 70.0; o->resolution = 0.5; o->leaf = 0.3f; o->reserved = 0;
    vgicp_default_options(&o->reg);
}

int vfront_create(int32_t device, int32_t max_scan_points, vfront_ctx** out) {
    if (!out || max_scan_points < 1 || max_scan_points > VF_MAX_POINTS) return VIL_ERR_INVALID_ARGUMENT;
    vfront_ctx* c = new vfront_ctx();
    c->msp = max_scan_points;
    const size_t N = (size_t)max_scan_points, nblk = (N + VF_BLK - 1) / VF_BLK;
    vilhost::Arena a;
    c->o_hdr = a.take(4 * H_INTS);
    c->o_raw = a.take(16 * N);
    c->o_tmp = a.take(16 * N);
    c->o_flag = a.take(4 * N);
    c->o_bcount = a.take(4 * nblk);
    c->o_kept = a.take(16 * N);
    c->o_filt = a.take(16 * N);
    c->o_xyz = a.take(12 * N);
    hipError_t err = c->open(device, a.bytes);
    if (err == hipSuccess) err = c->pin(&c->h_io, 16 * N);
    if (err == hipSuccess) err = c->pin(&c->h_hdr, 4 * H_INTS);
    int st = err == hipSuccess ? VIL_OK : VIL_ERR_DEVICE;
    if (st == VIL_OK) st = vcloud_create(device, max_scan_points, 1, &c->cloud);
    if (st == VIL_OK) st = vgicp_create(device, &c->reg);
    if (st == VIL_OK) st = vloop_create(device, max_scan_points, &c->loop);
    if (st != VIL_OK) { vfront_destroy(c); VILCHK(err); return st; }
    *out = c;
    return VIL_OK;
}

void vfront_destroy(vfront_ctx* c) {
    if (!c) return;
    vloop_destroy(c->loop); vgicp_destroy(c->reg); vcloud_destroy(c->cloud);
    c->close(c->prof);
    delete c;
}

int vfront_reset(vfront_ctx* c) {
    if (!c) return VIL_ERR_INVALID_ARGUMENT;
    c->has_prev = false; c->broken = false; c->last_kept = c->last_filt = 0;
    return VIL_OK;
}

int vfront_set_grid(vfront_ctx* c, int32_t min_points, double cell) {
    if (!c) return VIL_ERR_INVALID_ARGUMENT;
    return vloop_set_grid(c->loop, min_points, cell);
}

int vfront_profile_enable(vfront_ctx* c, int32_t enable) {
    if (!c) return VIL_ERR_INVALID_ARGUMENT;
    VILCHK(hipSetDevice(c->device));
    c->prof.on = enable != 0;
    return VIL_OK;
}
int vfront_profile_read(vfront_ctx* c, int64_t* launches4, double* total_ms4) {
    if (!c || !launches4 || !total_ms4) return VIL_ERR_INVALID_ARGUMENT;
    c->prof.read(launches4, total_ms4);
    return VIL_OK;
}

int vfront_push_scan(vfront_ctx* c, int32_t n, const float* xyzi, const vfront_motion* motion, const double* guess, const vfront_options* opts, vfront_summary* summary) {
    vfront_options o;
    vfront_default_options(&o);
    if (opts) o = *opts;
    if (!c || n < 0 || n > c->msp || (n && !xyzi) || !options_ok(o) || (o.deskew && !motion) || (guess && !finite_all(guess, 16))) return VIL_ERR_INVALID_ARGUMENT;
    Motion m = {1.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, (float)(1.0 / o.lidar_time_step)};
    if (o.deskew) {
        for (int k = 0; k < 4; ++k) if (!std::isfinite(motion->q[k])) return VIL_ERR_INVALID_ARGUMENT;
        for (int k = 0; k < 3; ++k) if (!std::isfinite(motion->t[k])) return VIL_ERR_INVALID_ARGUMENT;
        m.qw = motion->q[0]; m.qx = motion->q[1]; m.qy = motion->q[2]; m.qz = motion->q[3]; m.tx = motion->t[0]; m.ty = motion->t[1]; m.tz = motion->t[2];
    }
    if (c->broken) return VIL_ERR_DEVICE;

    VILCHK(hipSetDevice(c->device));
    int* hdr = c->at<int>(c->o_hdr);
    float4* d_kept = c->at<float4>(c->o_kept); float4* d_filt = c->at<float4>(c->o_filt);
    hipStream_t q = c->stream;
    const int nu = n > 0 ? n : 1, blocks = (nu + VF_BLK - 1) / VF_BLK;
    // steps 1 and 2: one submission over two streams and one host wait
    if (n) memcpy(c->h_io, xyzi, 16 * (size_t)n);
    VILCHK(hipMemsetAsync(hdr, 0, 4 * H_INTS, q));
    if (o.deskew) {
        float4* d_raw = c->at<float4>(c->o_raw); float4* d_tmp = c->at<float4>(c->o_tmp);
        int* d_flag = c->at<int>(c->o_flag); int* d_bcount = c->at<int>(c->o_bcount);
        if (n) VILCHK(hipMemcpyAsync(d_raw, c->h_io, 16 * (size_t)n, hipMemcpyHostToDevice, q));
        VILCHK(c->prof.mark(K_DESKEW, 1, q));
        hipLaunchKernelGGL(k_front_deskew, dim3(blocks), dim3(VF_BLK), 0, q, n, d_raw, m, o.min_distance, o.max_distance, d_tmp, d_flag, d_bcount);
        VILCHK(c->prof.mark(K_SCAN, 1, q));
        hipLaunchKernelGGL(k_front_scan, dim3(1), dim3(VF_BLK), 0, q, blocks, d_bcount, hdr + H_KEPT);
        VILCHK(c->prof.mark(K_SCATTER, 1, q));
        hipLaunchKernelGGL(k_front_scatter, dim3(blocks), dim3(VF_BLK), 0, q, n, d_tmp, d_flag, d_bcount, d_kept);
        VILCHK(c->prof.mark(-1, 0, q));
    } else {                                                                                        // the raw scan is the de-skewed cloud
        if (n) VILCHK(hipMemcpyAsync(d_kept, c->h_io, 16 * (size_t)n, hipMemcpyHostToDevice, q));
        VILCHK(hipMemsetD32Async((hipDeviceptr_t)(hdr + H_KEPT), n, 1, q));
    }
    VILCHK(c->ready.record(q));
    int st = vilcloud_stage::filter_resident(c->cloud, d_kept, hdr + H_KEPT, n, o.leaf, o.hist_size, d_filt, hdr + H_FILT, c->ready.ev, c->done);
    if (st != VIL_OK) return st;
    VILCHK(hipSetDevice(c->device));
    VILCHK(hipStreamWaitEvent(q, c->done.ev, 0));
    VILCHK(c->prof.mark(K_XYZ, 1, q));
    hipLaunchKernelGGL(k_front_xyz, dim3(blocks), dim3(VF_BLK), 0, q, hdr, n, d_filt, c->at<float>(c->o_xyz));
    VILCHK(c->prof.mark(-1, 0, q));
    VILCHK(hipMemcpyAsync(c->h_hdr, hdr, 4 * H_INTS, hipMemcpyDeviceToHost, q));
    VILCHK(hipStreamSynchronize(q));                                                                // host wait (1); it covers the filter's stream through `done`
    VILCHK(hipGetLastError());
    c->prof.collect();
    const int n_kept = c->h_hdr[H_KEPT], n_filt = c->h_hdr[H_FILT];
    if (n_kept < 0 || n_kept > n || n_filt < 0 || n_filt > n_kept) return VIL_ERR_DEVICE;
    c->last_kept = n_kept; c->last_filt = n_filt;

    vfront_summary s;
    memset(&s, 0, sizeof s);
    s.n_raw = n; s.n_kept = n_kept; s.n_filtered = n_filt;
    for (int k = 0; k < 4; ++k) s.T[5 * k] = 1.0;
    st = VIL_OK;
    if (n_filt && c->h_hdr[H_NONFINITE]) st = VIL_ERR_NON_FINITE;
    else if (n_filt) {
        st = exchange_and_align(c, n_filt, guess, o, s);
        if (st == VIL_ERR_DEVICE) c->broken = true;
    }
    if (summary) *summary = s;
    return st;
}

int vfront_read_deskewed(vfront_ctx* c, float* out_xyzi, int32_t capacity, int32_t* n) {
    if (!c) return VIL_ERR_INVALID_ARGUMENT;
    return read_points(c, c->o_kept, c->last_kept, out_xyzi, capacity, n);
}

int vfront_debug_read(vfront_ctx* c, int32_t stage, float* out_xyzi, int32_t capacity, int32_t* n) {
    if (!c) return VIL_ERR_INVALID_ARGUMENT;
    if (stage == VFRONT_DBG_DESKEWED) return read_points(c, c->o_kept, c->last_kept, out_xyzi, capacity, n);
    if (stage == VFRONT_DBG_FILTERED) return read_points(c, c->o_filt, c->last_filt, out_xyzi, capacity, n);
    return VIL_ERR_INVALID_ARGUMENT;
}

}  // extern "C"
