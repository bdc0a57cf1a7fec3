// vilsc.hip -- Scan Context place recognition on gfx950 behind include/vilsc.h
// (lidar_mapping/include/scancontext/Scancontext.cpp: SCManager; the steps are numbered as in the header).
//
// The database is resident: per entry 1200 floats (descriptor), 20 floats (ring key), 60 + 60 doubles (sector key, column norms).
// vsc_push_scan is one submission: the points go up, the 1200-word staging table is cleared on the stream, then
//   k_sc_bin     a thread per point (grid-stride): step 1.  A bin's maximum is an atomicMax on the order-preserving unsigned image of the
//                float, first in a workgroup-private table in LDS, then merged into the staging table the same way: the result does not
//                depend on the order the atomics arrive in.  Image 0 is no float's (it would be a NaN's): it marks an empty bin.
//   k_sc_finish  one workgroup: the -1000 rule, the descriptor, step 2's keys and norms, each sum by one thread in ascending order.
// vsc_detect is one submission and one read-back of a vsc_result:
//   k_sc_cand    (REFERENCE) a thread per searched entry, 1024 entries per workgroup: step 3's distance as a 64-bit key (distance bits <<
//                32 | index), then the workgroup's K smallest keys by K rounds of "smallest key not below the last winner + 1": keys are
//                unique, so no marking is needed and the rounds are deterministic.
//   k_sc_select  (REFERENCE) one workgroup merges the workgroups' lists into the candidate list by the same rounds.
//   k_sc_score   a workgroup per scored entry: query and entry in LDS; wave 0 does the sector-key pre-alignment (a lane per shift) and
//                lists the shifts to score; all threads fill the (shift, column) table of 20-term column dot products -- 420 of them in
//                REFERENCE mode, 3600 in EXHAUSTIVE mode; a lane per shift then sums its row in ascending column order.  Plain fp64
//                vector arithmetic: a product of two widened floats is exact, every sum has one defined order.
//   k_sc_decide  one workgroup: step 5 over the scored entries, the record.
// The arithmetic of the reference is kept unfused and in source order (x86 g++ and numpy do not contract a * b + c; hipcc would):
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/vilsc.h"
#include "vil_host.hpp"
#include "vil_math.hpp"

#define SC_R VSC_NUM_RING
#define SC_S VSC_NUM_SECTOR
#define SC_BINS (SC_R * SC_S)
#define SC_K VSC_MAX_CANDIDATES
#define SC_CHUNK 1024                // entries per workgroup of k_sc_cand: 4 per thread
#define SC_DOT_LD (SC_S + 1)         // row stride of the dot table in LDS (doubles): 61, so that the lanes of a row sum spread over the banks
#define SC_EMPTY (~0ull)
#define SC_BIG 10000000.0
#define SC_MAX_BIN_BLOCKS 512

namespace {

enum { K_BIN = 0, K_FINISH, K_CAND, K_SELECT, K_SCORE, K_DECIDE };

// order-preserving unsigned image of a non-NaN float (-0 below +0); 0 is not an image
__device__ __forceinline__ unsigned ord_of(const float v) { const unsigned u = __float_as_uint(v); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ float ord_back(const unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// step 1, :25-38
__device__ __forceinline__ float xy2theta(const float x, const float y) {
    const double k = 180.0 / M_PI;
    if (x >= 0.0f && y >= 0.0f) return (float)(k * atan((double)(y / x)));
    if (x < 0.0f && y >= 0.0f) return (float)(180.0 - k * atan((double)(y / (-x))));
    if (x < 0.0f && y < 0.0f) return (float)(180.0 + k * atan((double)(y / x)));
    return (float)(360.0 - k * atan((double)((-y) / x)));
}

__global__ __launch_bounds__(256) void k_sc_bin(int n, const float4* __restrict__ pts, double lidar_height, double max_radius, unsigned* __restrict__ stage) {
    __shared__ unsigned s_tab[SC_BINS];
    const int t = threadIdx.x;
    for (int i = t; i < SC_BINS; i += 256) s_tab[i] = 0u;
    __syncthreads();
    for (int i = blockIdx.x * 256 + t; i < n; i += gridDim.x * 256) {
        const float4 p = pts[i];
        if (!(isfinite(p.x) && isfinite(p.y)) || (p.x == 0.0f && p.y == 0.0f)) continue;           // DEVIATION of step 1
        const float zp = (float)((double)p.z + lidar_height);
        const float range = sqrtf(p.x * p.x + p.y * p.y);
        const float theta = xy2theta(p.x, p.y);
        if ((double)range > max_radius) continue;
        const int ring = max(min(SC_R, (int)ceil((double)range / max_radius * (double)SC_R)), 1);
        const int sector = max(min(SC_S, (int)ceil((double)theta / 360.0 * (double)SC_S)), 1);
        if (zp != zp) continue;                                                                     // a NaN never wins desc < z
        atomicMax(&s_tab[(ring - 1) * SC_S + (sector - 1)], ord_of(zp));                            // ring in [1, 20], sector in [1, 60]: inside the table
    }
    __syncthreads();
    for (int i = t; i < SC_BINS; i += 256) { const unsigned k = s_tab[i]; if (k) atomicMax(&stage[i], k); }
}

// raw != nullptr: a descriptor given by the caller (vsc_push_descriptor); otherwise the staging table
__global__ __launch_bounds__(256) void k_sc_finish(const unsigned* __restrict__ stage, const float* __restrict__ raw, int id, float* __restrict__ desc, float* __restrict__ ringkey,
                                                   double* __restrict__ sectkey, double* __restrict__ colnorm) {
    __shared__ float s_d[SC_BINS];
    const int t = threadIdx.x;
    for (int i = t; i < SC_BINS; i += 256) {
        float v;
        if (raw) v = raw[i];
        else {
            const unsigned k = stage[i], k0 = ord_of(-1000.0f);
            v = ord_back(k > k0 ? k : k0);
            if (v == -1000.0f) v = 0.0f;
        }
        s_d[i] = v;
        desc[(size_t)id * SC_BINS + i] = v;
    }
    __syncthreads();
    if (t < SC_R) {                                                                                // step 2, ring key
        double a = 0.0;
        for (int c = 0; c < SC_S; ++c) a = a + (double)s_d[t * SC_S + c];
        ringkey[(size_t)id * SC_R + t] = (float)(a / (double)SC_S);
    } else if (t >= 64 && t < 64 + SC_S) {                                                         // sector key and column norm
        const int c = t - 64;
        double a = 0.0, q = 0.0;
        for (int r = 0; r < SC_R; ++r) { const double v = (double)s_d[r * SC_S + c]; a = a + v; q = q + v * v; }
        sectkey[(size_t)id * SC_S + c] = a / (double)SC_R;
        colnorm[(size_t)id * SC_S + c] = sqrt(q);
    }
}

// minimum over a 256-thread workgroup; `slot` (4 words) must not be one of the two slots used by the two previous calls' readers:
// callers alternate between two slots, one barrier per call
__device__ __forceinline__ unsigned long long block_min64(unsigned long long v, unsigned long long* slot) {
    v = vd::wave_min64(v);
    if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long m = slot[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) m = slot[w] < m ? slot[w] : m;
    return m;
}

__global__ __launch_bounds__(256) void k_sc_cand(int n_search, int q_id, int kc, const float* __restrict__ ringkey, unsigned long long* __restrict__ part) {
    __shared__ unsigned long long s_w[2][4];
    __shared__ float s_q[SC_R];
    const int t = threadIdx.x;
    if (t < SC_R) s_q[t] = ringkey[(size_t)q_id * SC_R + t];
    __syncthreads();
    unsigned long long key[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int e = blockIdx.x * SC_CHUNK + u * 256 + t;
        key[u] = SC_EMPTY;
        if (e < n_search) {                                                                         // n_search <= count: inside the ring keys
            const float4* rk = (const float4*)(ringkey + (size_t)e * SC_R);                         // 80 B per entry: 16-byte aligned
            float acc = 0.0f;
#pragma unroll
            for (int v = 0; v < SC_R / 4; ++v) {
                const float4 k4 = rk[v];
                float d = s_q[4 * v] - k4.x; acc = acc + d * d;
                d = s_q[4 * v + 1] - k4.y; acc = acc + d * d;
                d = s_q[4 * v + 2] - k4.z; acc = acc + d * d;
                d = s_q[4 * v + 3] - k4.w; acc = acc + d * d;
            }
            const unsigned bits = acc != acc ? 0x7fc00000u : __float_as_uint(acc);                  // acc >= 0 orders like its bits; a NaN last
            key[u] = ((unsigned long long)bits << 32) | (unsigned)e;
        }
    }
    unsigned long long lo = 0ull;
    for (int r = 0; r < SC_K; ++r) {
        unsigned long long m = SC_EMPTY;
        if (r < kc) {                                                                               // uniform
#pragma unroll
            for (int u = 0; u < 4; ++u) if (key[u] >= lo && key[u] < m) m = key[u];
            m = block_min64(m, s_w[r & 1]);
            lo = m == SC_EMPTY ? SC_EMPTY : m + 1ull;
        }
        if (t == 0) part[(size_t)blockIdx.x * SC_K + r] = m;
    }
}

__global__ __launch_bounds__(256) void k_sc_select(int n_keys, int kc, const unsigned long long* __restrict__ part, int* __restrict__ cand) {
    __shared__ unsigned long long s_w[2][4];
    const int t = threadIdx.x;
    unsigned long long lo = 0ull;
    for (int r = 0; r < kc; ++r) {
        unsigned long long m = SC_EMPTY;
        for (int i = t; i < n_keys; i += 256) { const unsigned long long k = part[i]; if (k >= lo && k < m) m = k; }
        m = block_min64(m, s_w[r & 1]);
        lo = m == SC_EMPTY ? SC_EMPTY : m + 1ull;
        if (t == 0) cand[r] = m == SC_EMPTY ? 0 : (int)(unsigned)m;                                 // kc <= n_search keys exist: never empty
    }
}

// the lexicographic minimum of (v, i) over a wave; v is never a NaN here
__device__ __forceinline__ void wave_argmin(double& v, int& i) {
    for (int o = 32; o; o >>= 1) {
        const double w = __shfl_xor(v, o); const int j = __shfl_xor(i, o);
        if (w < v || (w == v && j < i)) { v = w; i = j; }
    }
}

__global__ __launch_bounds__(256) void k_sc_score(int mode, int q_id, int radius, const int* __restrict__ cand, const float* __restrict__ desc, const double* __restrict__ sectkey,
                                                  const double* __restrict__ colnorm, double* __restrict__ dist_out, int* __restrict__ shift_out) {
    __shared__ __align__(16) float s_q[SC_BINS], s_e[SC_BINS];
    __shared__ double s_dot[SC_S * SC_DOT_LD];
    __shared__ double s_nq[SC_S], s_ne[SC_S], s_vq[SC_S], s_ve[SC_S];
    __shared__ int s_list[SC_S];
    __shared__ int s_n;
    const int t = threadIdx.x, lane = t & 63;
    const int e = mode == VSC_MODE_REFERENCE ? cand[blockIdx.x] : (int)blockIdx.x;                 // an index below n_search <= count
    const float4* gq = (const float4*)(desc + (size_t)q_id * SC_BINS); const float4* ge = (const float4*)(desc + (size_t)e * SC_BINS);     // 4800 B per entry
    for (int i = t; i < SC_BINS / 4; i += 256) { ((float4*)s_q)[i] = gq[i]; ((float4*)s_e)[i] = ge[i]; }
    if (t < SC_S) { s_nq[t] = colnorm[(size_t)q_id * SC_S + t]; s_vq[t] = sectkey[(size_t)q_id * SC_S + t]; }
    else if (t >= 64 && t < 64 + SC_S) { s_ne[t - 64] = colnorm[(size_t)e * SC_S + t - 64]; s_ve[t - 64] = sectkey[(size_t)e * SC_S + t - 64]; }
    __syncthreads();
    if (t < 64) {                                                                                   // wave 0: the shifts to score, ascending
        bool in = lane < SC_S;
        if (mode == VSC_MODE_REFERENCE) {                                                           // fastAlignUsingVkey, a lane per shift
            double v = INFINITY; int a = 0;
            if (lane < SC_S) {
                double acc = 0.0;
                for (int j = 0; j < SC_S; ++j) { const int c = j - lane + (j < lane ? SC_S : 0); const double d = s_vq[j] - s_ve[c]; acc = acc + d * d; }
                const double nrm = sqrt(acc);
                if (nrm < SC_BIG) { v = nrm; a = lane; }                                            // strict < from 10000000: the first minimum
            }
            wave_argmin(v, a);
            const int dd = lane >= a ? lane - a : a - lane;
            in = in && min(dd, SC_S - dd) <= radius;
        }
        const unsigned long long b = __ballot(in);
        if (in) s_list[__popcll(b & ((1ull << lane) - 1ull))] = lane;                               // rank < 60
        if (lane == 0) s_n = __popcll(b);
    }
    __syncthreads();
    const int ns = s_n;
    for (int p = t; p < ns * SC_S; p += 256) {                                                      // dot[k][j]: query column j with entry column (j - s_k) mod 60
        const int k = p / SC_S, j = p - k * SC_S, s = s_list[k], c = j - s + (j < s ? SC_S : 0);
        double acc = 0.0;
#pragma unroll 4
        for (int r = 0; r < SC_R; ++r) acc = acc + (double)s_q[r * SC_S + j] * (double)s_e[r * SC_S + c];
        s_dot[k * SC_DOT_LD + j] = acc;
    }
    __syncthreads();
    if (t < 64) {                                                                                   // distDirectSC, a lane per shift
        double v = INFINITY; int sh = 0;
        if (lane < ns) {
            const int s = s_list[lane];
            double sum = 0.0; int cnt = 0;
            for (int j = 0; j < SC_S; ++j) {
                const int c = j - s + (j < s ? SC_S : 0);
                const double nq = s_nq[j], ne = s_ne[c];
                if (nq == 0.0 || ne == 0.0) continue;
                sum = sum + s_dot[lane * SC_DOT_LD + j] / (nq * ne);
                ++cnt;
            }
            const double dist = 1.0 - sum / (double)cnt;
            if (dist < SC_BIG) { v = dist; sh = s; }
        }
        wave_argmin(v, sh);
        if (lane == 0) { dist_out[blockIdx.x] = v == INFINITY ? SC_BIG : v; shift_out[blockIdx.x] = v == INFINITY ? 0 : sh; }
    }
}

__global__ __launch_bounds__(256) void k_sc_decide(int mode, int n_scored, int n_searched, double dist_thres, const int* __restrict__ cand, const double* __restrict__ dist,
                                                   const int* __restrict__ shift, vsc_result* __restrict__ res) {
    __shared__ double s_v[4];
    __shared__ int s_i[4];
    const int t = threadIdx.x;
    double v = INFINITY; int slot = 0;
    for (int i = t; i < n_scored; i += 256) { const double d = dist[i]; if (d < SC_BIG && d < v) { v = d; slot = i; } }      // ascending i: the first minimum
    if (v == INFINITY) slot = 0;
    wave_argmin(v, slot);
    if ((t & 63) == 0) { s_v[t >> 6] = v; s_i[t >> 6] = slot; }
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < 4; ++w) if (s_v[w] < v || (s_v[w] == v && s_i[w] < slot)) { v = s_v[w]; slot = s_i[w]; }
        vsc_result r;
        const bool any = v != INFINITY;
        r.min_dist = any ? v : SC_BIG;
        r.nn_idx = any ? (mode == VSC_MODE_REFERENCE ? cand[slot] : slot) : 0;
        r.nn_align = any ? shift[slot] : 0;
        r.loop_id = r.min_dist < dist_thres ? r.nn_idx : -1;
        r.n_searched = n_searched;
        r.yaw_diff_rad = (float)((double)(float)((double)r.nn_align * 6.0) * M_PI / 180.0);
        r.pad = 0;
        *res = r;
    }
}

bool config_ok(const vsc_config& c) {
    return std::isfinite(c.lidar_height) && std::isfinite(c.max_radius) && c.max_radius > 0.0 && !std::isnan(c.dist_thres) && c.search_ratio >= 0.0 && c.search_ratio <= 1.0 &&
           c.num_exclude_recent >= 0 && c.num_candidates >= 1 && c.num_candidates <= SC_K;
}

}  // namespace

struct vsc_ctx : vilhost::Device {           // d_mem: descriptors | ring keys | sector keys | norms | points | staging | raw | partial lists | candidates | dist | shift | record
    vsc_config cfg;
    int max_entries = 0, max_points = 0, count = 0, radius = 0, n_parts = 0;
    char* h_in = nullptr; vsc_result* h_res = nullptr;      // pinned: points or a descriptor up, the record down
    size_t o_desc = 0, o_ring = 0, o_sect = 0, o_norm = 0, o_pts = 0, o_stage = 0, o_raw = 0, o_part = 0, o_cand = 0, o_dist = 0, o_shift = 0, o_res = 0;
    int last_mode = 0, last_scored = 0;                     // what vsc_debug_read reads
    vilhost::Profiler<VSC_NUM_KERNELS, 5> prof;
};

namespace {
// the common tail of the two pushes: k_sc_finish appends entry `count`.  Events: [0] k_sc_bin [1] k_sc_finish [2]
int finish_push(vsc_ctx* c, const float* d_raw, bool with_bin, int32_t* id_out) {
    char* d = c->d_mem;
    hipLaunchKernelGGL(k_sc_finish, dim3(1), dim3(256), 0, c->stream, (const unsigned*)(d + c->o_stage), d_raw, c->count, (float*)(d + c->o_desc), (float*)(d + c->o_ring),
                       (double*)(d + c->o_sect), (double*)(d + c->o_norm));
    VILCHK(c->prof.mark(2, c->stream));
    VILCHK(hipStreamSynchronize(c->stream));                 // the pinned upload buffer is free again; nothing is read back
    VILCHK(hipGetLastError());
    if (with_bin) c->prof.span(K_BIN, 0, 1);
    c->prof.span(K_FINISH, 1, 2);
    if (id_out) *id_out = c->count;
    c->count++;
    return VIL_OK;
}
}  // namespace

extern "C" {

void vsc_default_config(vsc_config* cfg) {
    if (!cfg) return;
    cfg->lidar_height = 2.0; cfg->max_radius = 80.0; cfg->dist_thres = 0.5; cfg->search_ratio = 0.1; cfg->num_exclude_recent = 5; cfg->num_candidates = 3;
}

int vsc_create(int32_t device, int32_t max_entries, int32_t max_points, const vsc_config* cfg, vsc_ctx** out) {
    if (!out || max_entries < 1 || max_points < 1) return VIL_ERR_INVALID_ARGUMENT;
    vsc_config cf; vsc_default_config(&cf);
    if (cfg) cf = *cfg;
    if (!config_ok(cf)) return VIL_ERR_INVALID_ARGUMENT;
    vsc_ctx* c = new vsc_ctx();
    c->cfg = cf; c->max_entries = max_entries; c->max_points = max_points;
    c->radius = (int)std::round(0.5 * cf.search_ratio * (double)SC_S);
    c->n_parts = (max_entries + SC_CHUNK - 1) / SC_CHUNK;
    const size_t E = (size_t)max_entries, N = (size_t)max_points;
    vilhost::Arena a;
    c->o_desc = a.take(4 * SC_BINS * E);
    c->o_ring = a.take(4 * SC_R * E);
    c->o_sect = a.take(8 * SC_S * E);
    c->o_norm = a.take(8 * SC_S * E);
    c->o_pts = a.take(16 * N);
    c->o_stage = a.take(4 * SC_BINS);
    c->o_raw = a.take(4 * SC_BINS);
    c->o_part = a.take(8 * SC_K * (size_t)c->n_parts);
    c->o_cand = a.take(4 * SC_K);
    c->o_dist = a.take(8 * E);
    c->o_shift = a.take(4 * E);
    c->o_res = a.take(sizeof(vsc_result));
    const size_t h_in = 16 * N > 4 * (size_t)SC_BINS ? 16 * N : 4 * (size_t)SC_BINS;
    hipError_t err = c->open(device, a.bytes);
    if (err == hipSuccess) err = c->pin(&c->h_in, h_in);
    if (err == hipSuccess) err = c->pin(&c->h_res, sizeof(vsc_result));
    if (err != hipSuccess) { vsc_destroy(c); VILCHK(err); }
    *out = c;
    return VIL_OK;
}

void vsc_destroy(vsc_ctx* c) {
    if (!c) return;
    c->close(c->prof);
    delete c;
}

int vsc_profile_enable(vsc_ctx* c, int32_t enable) {
    if (!c) return VIL_ERR_INVALID_ARGUMENT;
    VILCHK(c->prof.enable(c->device, enable != 0));
    return VIL_OK;
}
int vsc_profile_read(vsc_ctx* c, int64_t* launches6, double* total_ms6) {
    if (!c || !launches6 || !total_ms6) return VIL_ERR_INVALID_ARGUMENT;
    c->prof.read(launches6, total_ms6);
    return VIL_OK;
}

int vsc_count(vsc_ctx* c) { return c ? c->count : VIL_ERR_INVALID_ARGUMENT; }
int vsc_reset(vsc_ctx* c) {
    if (!c) return VIL_ERR_INVALID_ARGUMENT;
    c->count = 0; c->last_scored = 0;
    return VIL_OK;
}

int vsc_push_scan(vsc_ctx* c, int32_t n, const float* xyzi, int32_t* id_out) {
    if (!c || n < 0 || n > c->max_points || (n && !xyzi) || c->count >= c->max_entries) return VIL_ERR_INVALID_ARGUMENT;
    VILCHK(hipSetDevice(c->device));
    char* d = c->d_mem;
    unsigned* d_stage = (unsigned*)(d + c->o_stage);
    if (n) {
        memcpy(c->h_in, xyzi, 16 * (size_t)n);
        VILCHK(hipMemcpyAsync(d + c->o_pts, c->h_in, 16 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    }
    VILCHK(hipMemsetAsync(d_stage, 0, 4 * SC_BINS, c->stream));
    VILCHK(c->prof.mark(0, c->stream));
    if (n) {
        const int blocks = (n + 255) / 256 < SC_MAX_BIN_BLOCKS ? (n + 255) / 256 : SC_MAX_BIN_BLOCKS;
        hipLaunchKernelGGL(k_sc_bin, dim3(blocks), dim3(256), 0, c->stream, n, (const float4*)(d + c->o_pts), c->cfg.lidar_height, c->cfg.max_radius, d_stage);
    }
    VILCHK(c->prof.mark(1, c->stream));
    return finish_push(c, nullptr, n > 0, id_out);
}

int vsc_push_descriptor(vsc_ctx* c, const float* desc, int32_t* id_out) {
    if (!c || !desc || c->count >= c->max_entries) return VIL_ERR_INVALID_ARGUMENT;
    VILCHK(hipSetDevice(c->device));
    memcpy(c->h_in, desc, 4 * SC_BINS);
    VILCHK(hipMemcpyAsync(c->d_mem + c->o_raw, c->h_in, 4 * SC_BINS, hipMemcpyHostToDevice, c->stream));
    VILCHK(c->prof.mark(1, c->stream));
    return finish_push(c, (const float*)(c->d_mem + c->o_raw), false, id_out);
}

int vsc_detect(vsc_ctx* c, int32_t mode, int32_t n_search, vsc_result* out) {
    if (!c || !out || (mode != VSC_MODE_REFERENCE && mode != VSC_MODE_EXHAUSTIVE) || n_search == 0 || n_search > c->count) return VIL_ERR_INVALID_ARGUMENT;
    c->last_mode = mode; c->last_scored = 0;
    if (c->count < c->cfg.num_exclude_recent + 1) {         // :349-353
        out->min_dist = SC_BIG; out->loop_id = -1; out->nn_idx = 0; out->nn_align = 0; out->n_searched = 0; out->yaw_diff_rad = 0.0f; out->pad = 0;
        return VIL_OK;
    }
    if (n_search < 0) n_search = c->count - c->cfg.num_exclude_recent;                             // >= 1
    VILCHK(hipSetDevice(c->device));
    char* d = c->d_mem;
    const int q = c->count - 1;
    const bool ref = mode == VSC_MODE_REFERENCE;
    const int kc = c->cfg.num_candidates < n_search ? c->cfg.num_candidates : n_search;
    const int n_scored = ref ? kc : n_search;
    int* d_cand = (int*)(d + c->o_cand); double* d_dist = (double*)(d + c->o_dist); int* d_shift = (int*)(d + c->o_shift);
    VILCHK(c->prof.mark(0, c->stream));
    if (ref) {
        const int parts = (n_search + SC_CHUNK - 1) / SC_CHUNK;                                     // <= n_parts
        hipLaunchKernelGGL(k_sc_cand, dim3(parts), dim3(256), 0, c->stream, n_search, q, kc, (const float*)(d + c->o_ring), (unsigned long long*)(d + c->o_part));
        VILCHK(c->prof.mark(1, c->stream));
        hipLaunchKernelGGL(k_sc_select, dim3(1), dim3(256), 0, c->stream, parts * SC_K, kc, (const unsigned long long*)(d + c->o_part), d_cand);
    } else VILCHK(c->prof.mark(1, c->stream));
    VILCHK(c->prof.mark(2, c->stream));
    hipLaunchKernelGGL(k_sc_score, dim3(n_scored), dim3(256), 0, c->stream, mode, q, c->radius, d_cand, (const float*)(d + c->o_desc), (const double*)(d + c->o_sect),
                       (const double*)(d + c->o_norm), d_dist, d_shift);
    VILCHK(c->prof.mark(3, c->stream));
    hipLaunchKernelGGL(k_sc_decide, dim3(1), dim3(256), 0, c->stream, mode, n_scored, n_search, c->cfg.dist_thres, d_cand, d_dist, d_shift, (vsc_result*)(d + c->o_res));
    VILCHK(c->prof.mark(4, c->stream));
    VILCHK(hipMemcpyAsync(c->h_res, d + c->o_res, sizeof(vsc_result), hipMemcpyDeviceToHost, c->stream));
    VILCHK(hipStreamSynchronize(c->stream));
    VILCHK(hipGetLastError());
    if (ref) { c->prof.span(K_CAND, 0, 1); c->prof.span(K_SELECT, 1, 2); }
    c->prof.span(K_SCORE, 2, 3); c->prof.span(K_DECIDE, 3, 4);
    *out = *c->h_res;
    c->last_scored = n_scored;
    return VIL_OK;
}

int vsc_read_entry(vsc_ctx* c, int32_t id, float* desc, float* ringkey20, double* sectorkey60) {
    if (!c || id < 0 || id >= c->count) return VIL_ERR_INVALID_ARGUMENT;
    VILCHK(hipSetDevice(c->device));
    if (desc) VILCHK(hipMemcpyAsync(desc, c->d_mem + c->o_desc + 4 * SC_BINS * (size_t)id, 4 * SC_BINS, hipMemcpyDeviceToHost, c->stream));
    if (ringkey20) VILCHK(hipMemcpyAsync(ringkey20, c->d_mem + c->o_ring + 4 * SC_R * (size_t)id, 4 * SC_R, hipMemcpyDeviceToHost, c->stream));
    if (sectorkey60) VILCHK(hipMemcpyAsync(sectorkey60, c->d_mem + c->o_sect + 8 * SC_S * (size_t)id, 8 * SC_S, hipMemcpyDeviceToHost, c->stream));
    VILCHK(hipStreamSynchronize(c->stream));
    return VIL_OK;
}

int vsc_debug_read(vsc_ctx* c, int32_t capacity, double* dist, int32_t* shift, int32_t* candidates) {
    if (!c || capacity < c->last_scored) return VIL_ERR_INVALID_ARGUMENT;
    const int n = c->last_scored;
    if (n == 0) return VIL_OK;
    VILCHK(hipSetDevice(c->device));
    if (dist) VILCHK(hipMemcpyAsync(dist, c->d_mem + c->o_dist, 8 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    if (shift) VILCHK(hipMemcpyAsync(shift, c->d_mem + c->o_shift, 4 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    if (candidates && c->last_mode == VSC_MODE_REFERENCE) VILCHK(hipMemcpyAsync(candidates, c->d_mem + c->o_cand, 4 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    VILCHK(hipStreamSynchronize(c->stream));
    if (candidates && c->last_mode != VSC_MODE_REFERENCE) for (int i = 0; i < n; ++i) candidates[i] = i;
    return VIL_OK;
}

}  // extern "C"
