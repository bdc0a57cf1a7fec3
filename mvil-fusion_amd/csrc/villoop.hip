// villoop.hip -- alignment fitness score and loop-closure verification on gfx950 behind include/villoop.h
// (pcl::Registration::getFitnessScore as estimator.cpp:303 and globalMappingIkdTree.cpp:512-573 use it; the steps are numbered as in the header).
//
// Both clouds are resident.  vloop_score is one submission and one read-back of n_T records; blockIdx.y is the transform:
//   k_loop_grid    a WAVE per source point: steps 1-3 through the uniform grid of vil_knn.hpp (knn_wave_query with k = 1: the 27 cells of a
//                  ring step are looked up by 27 lanes at once, the candidates are read 64 at a time in cell order); a query farther than
//                  KNN_RMAX cells from every target point ends in that function's exhaustive pass.
//   k_loop_brute   a LANE per source point, for small targets: the target streams through LDS 256 points at a time, every lane keeps the
//                  smallest (distance, index) key.  Same keys, same minimum: the same bits as k_loop_grid.
//   k_loop_sum     a workgroup per block of 256 consecutive source points: steps 4 and 5's partial, summed by one thread in ascending order.
//   k_loop_finish  a workgroup per transform: the partials in ascending order by one thread, the counts, the record.
// Nothing that feeds d2 may be contracted into an fma (x86 g++ and numpy do not contract a * b + c; hipcc would):
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/villoop.h"
#include "vil_host.hpp"
#include "vil_knn.hpp"
#include "villoop_stage.hpp"

#define VL_QPB 4                     // queries (waves) per workgroup of k_loop_grid
#define VL_BLK VLOOP_SUM_BLOCK

namespace {

using namespace vknn;

enum { K_GRID = 0, K_BRUTE, K_SUM, K_FINISH };

struct VlRec { double score; int n_used, pad; };

// steps 1 and 2: m = the float-rounded first three rows of T.  Contraction is off where the operations are written.
__device__ __forceinline__ void transform_point(const float* __restrict__ m, const float* __restrict__ p, float& qx, float& qy, float& qz) {
#pragma clang fp contract(off)
    const float x = p[0], y = p[1], z = p[2];
    qx = ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
    qy = ((m[4] * x + m[5] * y) + m[6] * z) + m[7];
    qz = ((m[8] * x + m[9] * y) + m[10] * z) + m[11];
}

__global__ __launch_bounds__(64 * VL_QPB) void k_loop_grid(int ns, const float* __restrict__ src, const float* __restrict__ T12, int nt, GridTab G, const int* __restrict__ order,
                                                           const float* __restrict__ cxyz, int stride, float* __restrict__ d2, int* __restrict__ idx) {
    __shared__ int wl_all[VL_QPB * KNN_WL_CAP];
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int i = blockIdx.x * VL_QPB + wave;
    if (i >= ns) return;                                                                            // wave-uniform; knn_wave_query has no workgroup barrier
    float qx, qy, qz;
    transform_point(T12 + 12 * blockIdx.y, src + 3 * (size_t)i, qx, qy, qz);
    unsigned long long best;
    knn_wave_query<true>(best, qx, qy, qz, 1, nt, G, order, cxyz, wl_all + wave * KNN_WL_CAP, 3.0e38f, 1);
    if (lane == 0) { d2[(size_t)blockIdx.y * stride + i] = knn_key_d(best); idx[(size_t)blockIdx.y * stride + i] = (int)(unsigned)best; }       // i < ns <= stride
}

__global__ __launch_bounds__(VL_BLK) void k_loop_brute(int ns, const float* __restrict__ src, const float* __restrict__ T12, int nt, const float* __restrict__ tgt, int stride,
                                                       float* __restrict__ d2, int* __restrict__ idx) {
    __shared__ float sx[VL_BLK], sy[VL_BLK], sz[VL_BLK];
    const int t = threadIdx.x, i = blockIdx.x * VL_BLK + t;
    const bool live = i < ns;
    float qx = 0.f, qy = 0.f, qz = 0.f;
    if (live) transform_point(T12 + 12 * blockIdx.y, src + 3 * (size_t)i, qx, qy, qz);
    unsigned long long best = ~0ull;
    for (int t0 = 0; t0 < nt; t0 += VL_BLK) {
        const int j0 = t0 + t;
        __syncthreads();
        if (j0 < nt) { sx[t] = tgt[3 * (size_t)j0]; sy[t] = tgt[3 * (size_t)j0 + 1]; sz[t] = tgt[3 * (size_t)j0 + 2]; }
        __syncthreads();
        const int cnt = min(VL_BLK, nt - t0);
        for (int jj = 0; jj < cnt; ++jj) {
            const unsigned long long key = knn_key(sqdist_strict(qx, qy, qz, sx[jj], sy[jj], sz[jj]), t0 + jj);
            best = key < best ? key : best;
        }
    }
    if (live) { d2[(size_t)blockIdx.y * stride + i] = knn_key_d(best); idx[(size_t)blockIdx.y * stride + i] = (int)(unsigned)best; }
}

// steps 4 and 5 for block blockIdx.x of transform blockIdx.y; an unused point is marked -1 (d2 is never negative)
__global__ __launch_bounds__(VL_BLK) void k_loop_sum(int ns, int stride, int pstride, double max_range, const float* __restrict__ d2, double* __restrict__ part, int* __restrict__ pcnt) {
    __shared__ double s_d[VL_BLK];
    const int t = threadIdx.x, i = blockIdx.x * VL_BLK + t;
    double v = -1.0;
    if (i < ns) { const double d = (double)d2[(size_t)blockIdx.y * stride + i]; if (d <= max_range) v = d; }
    s_d[t] = v;
    __syncthreads();
    if (t == 0) {
        double acc = 0.0; int cnt = 0;
#pragma unroll 16
        for (int j = 0; j < VL_BLK; ++j) { const double w = s_d[j]; const bool u = w >= 0.0; acc = acc + (u ? w : 0.0); cnt += u ? 1 : 0; }      // + 0.0 changes no bit of a sum >= 0
        part[(size_t)blockIdx.y * pstride + blockIdx.x] = acc; pcnt[(size_t)blockIdx.y * pstride + blockIdx.x] = cnt;       // blockIdx.x < nblk <= pstride
    }
}

__global__ __launch_bounds__(VL_BLK) void k_loop_finish(int nblk, int pstride, const double* __restrict__ part, const int* __restrict__ pcnt, VlRec* __restrict__ rec) {
    __shared__ double s_p[VL_BLK];
    __shared__ int s_c[VL_BLK];
    const int t = threadIdx.x;
    double acc = 0.0; int cnt = 0;
    for (int b0 = 0; b0 < nblk; b0 += VL_BLK) {
        __syncthreads();
        if (b0 + t < nblk) { s_p[t] = part[(size_t)blockIdx.x * pstride + b0 + t]; s_c[t] = pcnt[(size_t)blockIdx.x * pstride + b0 + t]; }
        __syncthreads();
        if (t == 0) { const int m = min(VL_BLK, nblk - b0); for (int j = 0; j < m; ++j) { acc = acc + s_p[j]; cnt += s_c[j]; } }
    }
    if (t == 0) { VlRec r; r.score = cnt ? acc / (double)cnt : DBL_MAX; r.n_used = cnt; r.pad = 0; rec[blockIdx.x] = r; }
}

bool all_finite(const float* xyz, size_t count) {
    for (size_t i = 0; i < count; ++i) if (!std::isfinite(xyz[i])) return false;
    return true;
}

}  // namespace

struct vloop_ctx : vilhost::Device {         // d_mem: target | source | transforms | d2 | idx | partials | counts | records
    int max_points = 0, pstride = 0, n_tgt = 0, n_src = 0;
    int grid_min = 1024; float grid_h = 0.5f; bool grid_valid = false;
    vknn::GridBuild gb;                     // grows on demand
    float* h_in = nullptr; float* h_T = nullptr; VlRec* h_rec = nullptr;       // pinned: a cloud up, the transforms up, the records down
    size_t o_tgt = 0, o_src = 0, o_T = 0, o_d2 = 0, o_idx = 0, o_part = 0, o_pcnt = 0, o_rec = 0;
    vilhost::Profiler<VLOOP_NUM_KERNELS, 4> prof;
};

namespace {

// n points at src (host memory, staged through the pinned buffer, or complete device memory) to the arena at off, and the wait for the copy
int upload_cloud(vloop_ctx* c, int32_t n, const float* src, size_t off, hipMemcpyKind kind) {
    VILCHK(hipSetDevice(c->device));
    if (kind == hipMemcpyHostToDevice) { memcpy(c->h_in, src, 12 * (size_t)n); src = c->h_in; }
    VILCHK(hipMemcpyAsync(c->d_mem + off, src, 12 * (size_t)n, kind, c->stream));
    VILCHK(hipStreamSynchronize(c->stream));                 // the pinned buffer is free again
    return VIL_OK;
}

int build_grid(vloop_ctx* c) {
    VILCHK(vknn::grid_build(c->gb, c->n_tgt, (const float*)(c->d_mem + c->o_tgt), 3, c->grid_h, c->stream));
    c->grid_valid = true;
    return VIL_OK;
}

// n points at src become the target: the old search structure dies with the old cloud, the new one is built when the cloud is large enough
int replace_target(vloop_ctx* c, int32_t n, const float* src, hipMemcpyKind kind) {
    c->grid_valid = false; c->n_tgt = 0;
    const int st = upload_cloud(c, n, src, c->o_tgt, kind);
    if (st != VIL_OK) return st;
    c->n_tgt = n;
    if (n >= c->grid_min) {
        const int sg = build_grid(c);
        if (sg != VIL_OK) return sg;
        VILCHK(hipStreamSynchronize(c->stream));
        VILCHK(hipGetLastError());
    }
    return VIL_OK;
}

// (R, t) -> (R^-1, -R^-1 t), bottom row 0 0 0 1; R^-1 by cofactors (R^T for an orthonormal R; a float-rounded R is one only to 6e-8)
void inverse_isometry(const double* T, double* D) {
    const double a = T[0], b = T[1], c = T[2], d = T[4], e = T[5], f = T[6], g = T[8], h = T[9], k = T[10];
    const double c00 = e * k - f * h, c01 = f * g - d * k, c02 = d * h - e * g;
    const double det = (a * c00 + b * c01) + c02 * c;
    const double inv[9] = {c00 / det, (c * h - b * k) / det, (b * f - c * e) / det, c01 / det, (a * k - c * g) / det, (c * d - a * f) / det,
                           c02 / det, (b * g - a * h) / det, (a * e - b * d) / det};
    for (int r = 0; r < 3; ++r) {
        for (int q = 0; q < 3; ++q) D[4 * r + q] = inv[3 * r + q];
        D[4 * r + 3] = -((inv[3 * r] * T[3] + inv[3 * r + 1] * T[7]) + inv[3 * r + 2] * T[11]);
    }
    D[12] = D[13] = D[14] = 0.0; D[15] = 1.0;
}

}  // namespace

int villoop_stage::install_source(vloop_ctx* c, int32_t n, const float* src, hipMemcpyKind kind) {
    if (!c || n < 1 || n > c->max_points || !src) return VIL_ERR_INVALID_ARGUMENT;
    c->n_src = 0;
    const int st = upload_cloud(c, n, src, c->o_src, kind);
    if (st != VIL_OK) return st;
    c->n_src = n;
    return VIL_OK;
}

int villoop_stage::promote_source(vloop_ctx* c) {
    if (!c || !c->n_src) return VIL_ERR_INVALID_ARGUMENT;
    return replace_target(c, c->n_src, (const float*)(c->d_mem + c->o_src), hipMemcpyDeviceToDevice);      // the source's copy was waited for
}

extern "C" {

int vloop_create(int32_t device, int32_t max_points, vloop_ctx** out) {
    if (!out || max_points <= 0) return VIL_ERR_INVALID_ARGUMENT;
    vloop_ctx* c = new vloop_ctx();
    c->max_points = max_points; c->pstride = (max_points + VL_BLK - 1) / VL_BLK;
    const size_t N = (size_t)max_points, B = VLOOP_MAX_BATCH, P = (size_t)c->pstride;
    vilhost::Arena a;
    c->o_tgt = a.take(12 * N);
    c->o_src = a.take(12 * N);
    c->o_T = a.take(4 * 12 * B);
    c->o_d2 = a.take(4 * N * B);
    c->o_idx = a.take(4 * N * B);
    c->o_part = a.take(8 * P * B);
    c->o_pcnt = a.take(4 * P * B);
    c->o_rec = a.take(sizeof(VlRec) * B);
    hipError_t err = c->open(device, a.bytes);
    if (err == hipSuccess) err = c->pin(&c->h_in, 12 * N);
    if (err == hipSuccess) err = c->pin(&c->h_T, 4 * 12 * B);
    if (err == hipSuccess) err = c->pin(&c->h_rec, sizeof(VlRec) * B);
    if (err != hipSuccess) { vloop_destroy(c); VILCHK(err); }
    *out = c;
    return VIL_OK;
}

void vloop_destroy(vloop_ctx* c) {
    if (!c) return;
    c->close(c->prof);
    delete c;
}

void vloop_default_options(vloop_options* o) {
    if (!o) return;
    vgicp_default_options(&o->reg);
    o->resolution = 0.5; o->max_tolerable_fitness = 1.0f; o->pad = 0;
}

int vloop_profile_enable(vloop_ctx* c, int32_t enable) {
    if (!c) return VIL_ERR_INVALID_ARGUMENT;
    VILCHK(c->prof.enable(c->device, enable != 0));
    return VIL_OK;
}
int vloop_profile_read(vloop_ctx* c, int64_t* launches4, double* total_ms4) {
    if (!c || !launches4 || !total_ms4) return VIL_ERR_INVALID_ARGUMENT;
    c->prof.read(launches4, total_ms4);
    return VIL_OK;
}

int vloop_set_grid(vloop_ctx* c, int32_t min_points, double cell) {
    if (!c || min_points < 0 || !(cell > 0.0) || !std::isfinite(cell)) return VIL_ERR_INVALID_ARGUMENT;
    c->grid_min = min_points; c->grid_h = (float)cell; c->grid_valid = false;
    return VIL_OK;
}

int vloop_set_target(vloop_ctx* c, int32_t n, const float* xyz) {
    if (!c || n < 1 || n > c->max_points || !xyz) return VIL_ERR_INVALID_ARGUMENT;
    if (!all_finite(xyz, 3 * (size_t)n)) return VIL_ERR_NON_FINITE;
    return replace_target(c, n, xyz, hipMemcpyHostToDevice);
}

int vloop_set_source(vloop_ctx* c, int32_t n, const float* xyz) {
    if (!c || n < 1 || n > c->max_points || !xyz) return VIL_ERR_INVALID_ARGUMENT;
    if (!all_finite(xyz, 3 * (size_t)n)) return VIL_ERR_NON_FINITE;
    return villoop_stage::install_source(c, n, xyz, hipMemcpyHostToDevice);
}

int vloop_score(vloop_ctx* c, int32_t n_T, const double* T16s, double max_range, double* scores, int32_t* n_used, float* nn_d2, int32_t* nn_idx) {
    if (!c || n_T < 1 || n_T > VLOOP_MAX_BATCH || !T16s || !scores || !c->n_src || !c->n_tgt || std::isnan(max_range)) return VIL_ERR_INVALID_ARGUMENT;
    for (int k = 0; k < n_T; ++k)
        for (int q = 0; q < 12; ++q) {
            const double v = T16s[16 * k + q];
            if (!std::isfinite(v)) return VIL_ERR_NON_FINITE;
            c->h_T[12 * k + q] = (float)v;                                                          // step 1
        }
    VILCHK(hipSetDevice(c->device));
    char* d = c->d_mem;
    const int ns = c->n_src, nt = c->n_tgt, stride = c->max_points, nblk = (ns + VL_BLK - 1) / VL_BLK;
    const float* d_src = (const float*)(d + c->o_src); const float* d_T = (const float*)(d + c->o_T);
    float* d_d2 = (float*)(d + c->o_d2); int* d_idx = (int*)(d + c->o_idx);
    double* d_part = (double*)(d + c->o_part); int* d_pcnt = (int*)(d + c->o_pcnt);
    const bool grid = nt >= c->grid_min;
    if (grid && !c->grid_valid) { const int sg = build_grid(c); if (sg != VIL_OK) return sg; }     // vloop_set_grid after vloop_set_target
    VILCHK(hipMemcpyAsync(d + c->o_T, c->h_T, 4 * 12 * (size_t)n_T, hipMemcpyHostToDevice, c->stream));
    VILCHK(c->prof.mark(0, c->stream));
    if (grid) hipLaunchKernelGGL(k_loop_grid, dim3((ns + VL_QPB - 1) / VL_QPB, n_T), dim3(64 * VL_QPB), 0, c->stream, ns, d_src, d_T, nt, c->gb.G, c->gb.order, c->gb.cxyz, stride, d_d2, d_idx);
    else hipLaunchKernelGGL(k_loop_brute, dim3(nblk, n_T), dim3(VL_BLK), 0, c->stream, ns, d_src, d_T, nt, (const float*)(d + c->o_tgt), stride, d_d2, d_idx);
    VILCHK(c->prof.mark(1, c->stream));
    hipLaunchKernelGGL(k_loop_sum, dim3(nblk, n_T), dim3(VL_BLK), 0, c->stream, ns, stride, c->pstride, max_range, d_d2, d_part, d_pcnt);
    VILCHK(c->prof.mark(2, c->stream));
    hipLaunchKernelGGL(k_loop_finish, dim3(n_T), dim3(VL_BLK), 0, c->stream, nblk, c->pstride, d_part, d_pcnt, (VlRec*)(d + c->o_rec));
    VILCHK(c->prof.mark(3, c->stream));
    VILCHK(hipMemcpyAsync(c->h_rec, d + c->o_rec, sizeof(VlRec) * (size_t)n_T, hipMemcpyDeviceToHost, c->stream));
    for (int k = 0; k < n_T; ++k) {                                                                 // debug outputs: row k of the strided tables
        if (nn_d2) VILCHK(hipMemcpyAsync(nn_d2 + (size_t)k * ns, d_d2 + (size_t)k * stride, 4 * (size_t)ns, hipMemcpyDeviceToHost, c->stream));
        if (nn_idx) VILCHK(hipMemcpyAsync(nn_idx + (size_t)k * ns, d_idx + (size_t)k * stride, 4 * (size_t)ns, hipMemcpyDeviceToHost, c->stream));
    }
    VILCHK(hipStreamSynchronize(c->stream));
    VILCHK(hipGetLastError());
    c->prof.span(grid ? K_GRID : K_BRUTE, 0, 1); c->prof.span(K_SUM, 1, 2); c->prof.span(K_FINISH, 2, 3);
    for (int k = 0; k < n_T; ++k) { scores[k] = c->h_rec[k].score; if (n_used) n_used[k] = c->h_rec[k].n_used; }
    return VIL_OK;
}

int vloop_verify(vloop_ctx* c, vgicp_ctx* reg, int32_t n_query, const float* query_xyz, int32_t n_cand, const vloop_candidate* cands, const vloop_options* o, vloop_best* best,
                 vloop_candidate_result* per) {
    if (!c || !reg || !query_xyz || !o || !best || n_cand < 0 || (n_cand && !cands) || n_query < 1 || n_query > c->max_points || !(o->resolution > 0.0) ||
        std::isnan(o->max_tolerable_fitness))
        return VIL_ERR_INVALID_ARGUMENT;
    for (int k = 0; k < n_cand; ++k) {
        if (cands[k].n < 1 || cands[k].n > c->max_points || !cands[k].xyz) return VIL_ERR_INVALID_ARGUMENT;
        for (int q = 0; q < 16; ++q) if (!std::isfinite(cands[k].guess[q])) return VIL_ERR_NON_FINITE;
    }
    best->index = -1; best->fitness = o->max_tolerable_fitness; best->n_used = 0; best->pad = 0;
    for (int q = 0; q < 16; ++q) best->T[q] = best->delta[q] = (q % 5 == 0) ? 1.0 : 0.0;
    int st = vloop_set_source(c, n_query, query_xyz);
    if (st == VIL_OK && n_cand) st = vgicp_set_source(reg, n_query, query_xyz, nullptr);
    if (st != VIL_OK) return st;
    float running = o->max_tolerable_fitness;                                                       // fitnessMinResult, :443
    for (int k = 0; k < n_cand; ++k) {
        const vloop_candidate& cd = cands[k];
        if ((st = vgicp_set_target(reg, cd.n, cd.xyz, nullptr, o->resolution)) != VIL_OK) return st;
        if ((st = vloop_set_target(c, cd.n, cd.xyz)) != VIL_OK) return st;
        double guess[16], T[16];
        for (int q = 0; q < 16; ++q) guess[q] = (double)(float)cd.guess[q];                         // Matrix4f init_guss, :555-557
        vgicp_summary sm;
        if ((st = vgicp_align(reg, guess, &o->reg, T, &sm)) != VIL_OK) return st;
        vloop_candidate_result r;
        r.converged = sm.converged; r.fitness = FLT_MAX; r.n_used = 0; r.iterations = sm.iterations;
        for (int q = 0; q < 16; ++q) r.T[q] = (double)(float)T[q];                                  // getFinalTransformation() is a Matrix4f
        if (sm.converged) {                                                                         // :560
            double score = 0.0; int32_t used = 0;
            if ((st = vloop_score(c, 1, r.T, DBL_MAX, &score, &used, nullptr, nullptr)) != VIL_OK) return st;
            r.fitness = (float)score; r.n_used = used;                                              // float fitnessScore, :564
            if (r.fitness < running) {                                                              // :477
                running = r.fitness;
                best->index = k; best->fitness = r.fitness; best->n_used = used;
                memcpy(best->T, r.T, sizeof r.T);
                inverse_isometry(r.T, best->delta);
            }
        }
        if (per) per[k] = r;
    }
    return VIL_OK;
}

}  // extern "C"
