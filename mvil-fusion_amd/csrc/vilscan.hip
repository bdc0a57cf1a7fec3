// vilscan.hip -- LOAM feature extraction of a raw LiDAR scan on gfx950 behind include/vilscan.h
// (lidar_mapping/src/scanRegistration.cpp: PointToRing :293-416, ExtractFeaturePoints :50-169, PrepareRing :510-561,
// PrepareSubregion :563-621, MaskPickedInRing :623-649; lidar_compensator/src/math_utils.h :62-91).
//
// One call is one submission of four kernels:
//   k_scan_ring_id    a thread per raw point: its ring (one byte), 0xff = dropped
//   k_scan_ring_sort  a workgroup per ring: counts the points of the rings below it and of its own (its slice of the ring table), then
//                     streams the ring bytes once more and places its points by ballot + popcount prefix -- a stable partition without
//                     atomics: the order of the output is part of the contract
//   k_scan_features   a workgroup per ring, the ring in LDS: mask, curvature and vote of every point in parallel, ONE bitonic sort of the
//                     whole ring on the key (subregion, curvature bits, index) -- the sorted subregions lie one after the other --, then
//                     wave 0 walks the subregions in order, 64 sorted candidates per step, first qualifying lane from the ballot; then the
//                     less-flat compaction and the exact voxel filter (LDS hash -> cell's first point, a second bitonic sort on
//                     (first point, point) that lines every cell up in emission order, one thread per cell sums in double in ring order)
//   k_scan_gather     a workgroup per ring: the rings' feature segments packed one after the other
// The float arithmetic of the reference is kept unfused and in source order (x86 g++ and numpy do not contract a * b + c; hipcc would):
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/vilscan.h"
#include "vil_host.hpp"

#define VS_CAP VSCAN_MAX_RING_POINTS
#define VS_THREADS 1024
#define VS_WAVES (VS_THREADS / 64)
#define VS_HASH (2 * VS_CAP)
#define VS_EMPTY 0x7fffffff
#define VS_OUTSIDE 3                 // label of a point that belongs to no processed subregion (reported as 0)
#define VS_MAX_SUB 256

namespace {
using vilhost::up16;

struct ScanP {
    int R, S, C, max_sharp, max_less, max_flat;
    float th_hi, th_lo, inv_leaf;          // surf_curv_th / 2, surf_curv_th / 10, 1 / less_flat_filter_size: float, rounded on the host
    double lower, factor;                  // ElevationToRing
};
// header of the result block (ints)
enum { H_NVALID = 0, H_SHARP, H_LESS, H_FLAT, H_LFDS, H_LFRAW, H_OVER, H_INTS = 16 };
// per-ring counts (ints)
enum { RC_SHARP = 0, RC_LESS, RC_FLAT, RC_LFDS, RC_LFRAW, RC_INTS = 8 };

__device__ __forceinline__ float sqdiff(const float4 a, const float4 b) {                 // CalcSquaredDiff(a, b)
    const float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
    return dx * dx + dy * dy + dz * dz;
}
__device__ __forceinline__ float sqdiff_w(const float4 a, const float4 b, const float wb) {   // CalcSquaredDiff(a, b, wb)
    const float dx = a.x - b.x * wb, dy = a.y - b.y * wb, dz = a.z - b.z * wb;
    return dx * dx + dy * dy + dz * dz;
}
__device__ __forceinline__ float sqnorm(const float4 p) { return p.x * p.x + p.y * p.y + p.z * p.z; }

__global__ __launch_bounds__(256) void k_scan_ring_id(int n, int npad, const float4* __restrict__ raw, unsigned char* __restrict__ id, ScanP P) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= npad) return;
    unsigned char r = 0xff;
    if (i < n) {
        const float4 p = raw[i];
        if (isfinite(p.x) && isfinite(p.y) && isfinite(p.z)) {
            const float dis = sqrtf(p.x * p.x + p.y * p.y);
            const float ele = atan2f(p.z, dis);
            const double v = ((double)ele * 180.0 / M_PI - P.lower) * P.factor + 0.5;
            if (v > -1.0 && v < (double)P.R) r = (unsigned char)(int)v;
        }
    }
    id[i] = r;
}

// exclusive rank of this thread's flag among the workgroup's flags, in thread order; total = number of flags.  s_w: VS_WAVES ints the
// caller alternates between two of (one barrier per call)
__device__ __forceinline__ int block_rank(const bool f, int& total, volatile int* s_w) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long b = __ballot(f);
    if (lane == 0) s_w[wave] = __popcll(b);
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < VS_WAVES; ++w) { const int c = s_w[w]; off += w < wave ? c : 0; tot += c; }
    total = tot;
    return off + __popcll(b & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(VS_THREADS) void k_scan_ring_sort(int npad, const float4* __restrict__ raw, const unsigned char* __restrict__ id, int* __restrict__ table,
                                                               float4* __restrict__ cloud, int* __restrict__ hdr) {
    __shared__ int s_w[2][VS_WAVES], s_red[2][VS_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n4 = npad >> 2;
    const unsigned r = blockIdx.x;
    const uint32_t* id4 = (const uint32_t*)id;
    int lo = 0, eq = 0;
    for (int w = tid; w < n4; w += VS_THREADS) {
        const uint32_t u = id4[w];
#pragma unroll
        for (int b = 0; b < 4; ++b) { const unsigned c = (u >> (8 * b)) & 0xffu; lo += c < r; eq += c == r; }
    }
    for (int o = 32; o; o >>= 1) { lo += __shfl_xor(lo, o); eq += __shfl_xor(eq, o); }
    if (lane == 0) { s_red[0][wave] = lo; s_red[1][wave] = eq; }
    __syncthreads();
    int start = 0, cnt = 0;
#pragma unroll
    for (int w = 0; w < VS_WAVES; ++w) { start += s_red[0][w]; cnt += s_red[1][w]; }
    if (tid == 0) {
        table[2 * r] = start; table[2 * r + 1] = cnt;
        if (r + 1 == gridDim.x) hdr[H_NVALID] = start + cnt;
        if (r == 0) hdr[H_OVER] = 0;
    }
    int base = start, par = 0;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int w0 = 0; w0 < n4; w0 += VS_THREADS, par ^= 1) {
        const int w = w0 + tid;
        const uint32_t u = w < n4 ? id4[w] : 0xffffffffu;
        bool f[4]; int before = 0, mine = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            f[b] = ((u >> (8 * b)) & 0xffu) == r;
            const unsigned long long bb = __ballot(f[b]);
            before += __popcll(bb & below); mine += __popcll(bb);
        }
        if (lane == 0) s_w[par][wave] = mine;
        __syncthreads();
        int off = 0, tot = 0;
#pragma unroll
        for (int v = 0; v < VS_WAVES; ++v) { const int c = s_w[par][v]; off += v < wave ? c : 0; tot += c; }
        int pos = base + off + before;
#pragma unroll
        for (int b = 0; b < 4; ++b) if (f[b]) cloud[pos++] = raw[4 * w + b];       // pos < start + cnt: the same bytes were counted above
        base += tot;
    }
}

template <class K>
__device__ __forceinline__ void lds_bitonic(K* a, const int N, const int tid) {       // ascending, N a power of two >= 2; ends on a barrier
    for (int k = 2; k <= N; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (N >> 1); t += VS_THREADS) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
                const K x = a[i], y = a[p];
                if ((x > y) == ((i & k) == 0)) { a[i] = y; a[p] = x; }
            }
            __syncthreads();
        }
}

__device__ __forceinline__ void cell_of(const float4 p, const float inv, int& cx, int& cy, int& cz) {
    cx = (int)floorf(p.x * inv); cy = (int)floorf(p.y * inv); cz = (int)floorf(p.z * inv);
}

// MaskPickedInRing by one wave: lane k (1..C) tests the gap between neighbours k - 1 and k on either side, the first gap ends the run
__device__ __forceinline__ void mask_picked(const float4* s_pt, signed char* s_mask, const int idx, const int C, const int lane) {
    const bool act = lane >= 1 && lane <= C;
    const bool gf = act && (double)sqdiff(s_pt[idx + lane], s_pt[idx + lane - 1]) > 0.05;
    const bool gb = act && (double)sqdiff(s_pt[idx - lane], s_pt[idx - lane + 1]) > 0.05;
    const unsigned long long bf = __ballot(gf), bb = __ballot(gb);
    const int nf = bf ? __ffsll((long long)bf) - 2 : C, nb = bb ? __ffsll((long long)bb) - 2 : C;      // ffs is 1-based: first gap at lane g masks lanes 1..g-1
    if (act && lane <= nf) s_mask[idx + lane] = 1;
    if (act && lane <= nb) s_mask[idx - lane] = 1;
    if (lane == 0) s_mask[idx] = 1;
    __builtin_amdgcn_wave_barrier();
}

__global__ __launch_bounds__(VS_THREADS) void k_scan_features(ScanP P, const int* __restrict__ table, const float4* __restrict__ cloud, signed char* __restrict__ labels,
                                                              float4* __restrict__ st_sharp, float4* __restrict__ st_less, float4* __restrict__ st_flat, float4* __restrict__ st_lf,
                                                              int* __restrict__ ring_cnt, int* __restrict__ hdr) {
    __shared__ float4 s_pt[VS_CAP];                          // 64 kB
    __shared__ unsigned long long s_key[VS_CAP];             // 32 kB; after the picks: s_lf | s_slot | s_k32
    __shared__ int s_hash[VS_HASH];                          // 32 kB
    __shared__ signed char s_mask[VS_CAP], s_label[VS_CAP];  // 8 kB
    __shared__ int s_sp[VS_MAX_SUB + 1], s_w[2][VS_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, r = blockIdx.x;
    const int start = table[2 * r], n = table[2 * r + 1], C = P.C, S = P.S;
    int* cnt = ring_cnt + RC_INTS * r;
    if (n > VS_CAP || n <= 2 * C + 1) {                      // over the LDS plan (the host reports it) / "skip too short scans" (:64)
        if (tid < RC_INTS) cnt[tid] = 0;
        if (tid == 0 && n > VS_CAP) hdr[H_OVER] = 1;
        for (int i = tid; i < n; i += VS_THREADS) labels[start + i] = 0;
        return;
    }
    int P2 = 2; while (P2 < n) P2 <<= 1;
    for (int i = tid; i < n; i += VS_THREADS) { s_pt[i] = cloud[start + i]; s_mask[i] = 0; s_label[i] = VS_OUTSIDE; }
    if (tid <= S) s_sp[tid] = C + (int)(((size_t)tid * (size_t)(n - 2 * C)) / (size_t)S);         // sp of :78; ep = s_sp[j + 1] - 1
    __syncthreads();
    for (int i = tid; i < P2; i += VS_THREADS) {
        unsigned long long key = ~0ull;
        if (i >= C && i < n - C) {
            const float4 pc = s_pt[i], pn = s_pt[i + 1], pp = s_pt[i - 1];
            {   // PrepareRing (:510-561)
                const float diff_next2 = sqdiff(pc, pn);
                bool done = false;
                if ((double)diff_next2 > 0.1) {
                    const float depth = sqrtf(sqnorm(pc)), depth_next = sqrtf(sqnorm(pn));
                    if (depth > depth_next) {
                        const float wd = sqrtf(sqdiff_w(pn, pc, depth_next / depth)) / depth_next;
                        if ((double)wd < 0.1) { for (int k = 0; k <= C; ++k) s_mask[i - C + k] = 1; done = true; }
                    } else {
                        const float wd = sqrtf(sqdiff_w(pc, pn, depth / depth_next)) / depth;
                        if ((double)wd < 0.1) { for (int k = 1; k <= C + 1; ++k) if (i + k < n) s_mask[i + k] = 1; done = true; }    // clamped to the ring (vilscan.h)
                    }
                }
                if (!done) {
                    const float diff_prev2 = sqdiff(pc, pp), dis2 = sqnorm(pc);
                    if ((double)diff_next2 > 0.0002 * (double)dis2 && (double)diff_prev2 > 0.0002 * (double)dis2) s_mask[i] = 1;
                }
            }
            // subregion of i: the largest j with sp_j <= i
            int j = (int)(((size_t)(i - C) * (size_t)S) / (size_t)(n - 2 * C));
            while (j + 1 < S && s_sp[j + 1] <= i) ++j;
            while (j > 0 && s_sp[j] > i) --j;
            if (s_sp[j + 1] - 1 > s_sp[j]) {                 // "skip empty regions" (ep <= sp)
                // PrepareSubregion (:563-621)
                const float nn = (float)(-2 * C);
                float dx = nn * pc.x, dy = nn * pc.y, dz = nn * pc.z;
                int vote = 0;
                for (int k = 1; k <= C; ++k) {
                    const float4 a = s_pt[i + k], b = s_pt[i - k];
                    dx += a.x + b.x; dy += a.y + b.y; dz += a.z + b.z;
                    const float ra = a.w / pc.w, rb = b.w / pc.w;
                    vote += (ra >= 1.0f && ra < 2.0f) ? 1 : 0;
                    vote += (rb >= 1.0f && rb < 2.0f) ? 1 : 0;
                }
                const float curv = dx * dx + dy * dy + dz * dz;
                if (curv > P.th_hi && vote > 4) s_mask[i] = 1;
                else if (curv < P.th_lo && vote < 5) s_mask[i] = 1;
                s_label[i] = 0;
                key = ((unsigned long long)j << 48) | ((unsigned long long)__float_as_uint(curv) << 16) | (unsigned long long)i;
            }
        }
        s_key[i] = key;
    }
    __syncthreads();
    lds_bitonic(s_key, P2, tid);
    if (tid < 64) {                                          // the picks (:90-146): the mask is the ring's, so its subregions go in order
        int n_sharp = 0, n_less = 0, n_flat = 0, off = 0;
        float4* o_sharp = st_sharp + (size_t)r * S * P.max_sharp; float4* o_less = st_less + (size_t)r * S * P.max_less; float4* o_flat = st_flat + (size_t)r * S * P.max_flat;
        for (int j = 0; j < S; ++j) {
            const int size = s_sp[j + 1] - s_sp[j];
            if (size < 2) continue;
            int picked = 0, pos = off + size - 1;
            while (picked < P.max_less && pos >= off) {      // from the high end
                const int cand = pos - lane; const bool valid = cand >= off;
                const unsigned long long key = valid ? s_key[cand] : 0ull;
                const int idx = (int)(key & 0xffffull);
                const bool big = valid && __uint_as_float((unsigned)(key >> 16)) > P.th_hi;
                const unsigned long long bq = __ballot(big && s_mask[idx] == 0);
                if (!bq) { if (__ballot(valid && !big)) break; pos -= 64; continue; }       // sorted: nothing below a failed curvature test can pass it
                const int f = __ffsll((long long)bq) - 1, pidx = __shfl(idx, f);
                ++picked;
                if (lane == 0) {
                    const float4 p = s_pt[pidx];
                    if (picked <= P.max_sharp) { s_label[pidx] = 2; o_sharp[n_sharp] = p; } else s_label[pidx] = 1;
                    o_less[n_less] = p;
                }
                if (picked <= P.max_sharp) ++n_sharp;
                ++n_less;
                mask_picked(s_pt, s_mask, pidx, C, lane);
                pos -= f + 1;
            }
            picked = 0; pos = off;
            const int end = off + size;
            while (picked < P.max_flat && pos < end) {       // from the low end
                const int cand = pos + lane; const bool valid = cand < end;
                const unsigned long long key = valid ? s_key[cand] : 0ull;
                const int idx = (int)(key & 0xffffull);
                const bool small = valid && __uint_as_float((unsigned)(key >> 16)) < P.th_lo;
                const unsigned long long bq = __ballot(small && s_mask[idx] == 0);
                if (!bq) { if (__ballot(valid && !small)) break; pos += 64; continue; }
                const int f = __ffsll((long long)bq) - 1, pidx = __shfl(idx, f);
                ++picked;
                if (lane == 0) { s_label[pidx] = -1; o_flat[n_flat] = s_pt[pidx]; }
                ++n_flat;
                mask_picked(s_pt, s_mask, pidx, C, lane);
                pos += f + 1;
            }
            off += size;
        }
        if (lane == 0) { cnt[RC_SHARP] = n_sharp; cnt[RC_LESS] = n_less; cnt[RC_FLAT] = n_flat; }
    }
    __syncthreads();
    // ---- less flat: every point of a processed subregion with label <= 0, in index order (the keys are no longer needed)
    unsigned short* s_lf = (unsigned short*)s_key; unsigned short* s_slot = s_lf + VS_CAP; unsigned* s_k32 = (unsigned*)(s_slot + VS_CAP);
    int m = 0, par = 0;
    for (int c0 = 0; c0 < n; c0 += VS_THREADS, par ^= 1) {
        const int i = c0 + tid;
        signed char lab = VS_OUTSIDE;
        if (i < n) { lab = s_label[i]; labels[start + i] = lab == VS_OUTSIDE ? 0 : lab; }
        int tot;
        const int rk = block_rank(lab <= 0, tot, s_w[par]);
        if (lab <= 0) s_lf[m + rk] = (unsigned short)i;
        m += tot;
    }
    for (int h = tid; h < VS_HASH; h += VS_THREADS) s_hash[h] = VS_EMPTY;
    __syncthreads();
    // ---- exact voxel filter.  A table slot is a cell; its value is the cell's first point so far (always a member of the cell, so it
    //      also identifies the cell).  Which slot a cell gets may depend on timing, what comes out does not.
    for (int q = tid; q < m; q += VS_THREADS) {
        int cx, cy, cz; cell_of(s_pt[s_lf[q]], P.inv_leaf, cx, cy, cz);
        unsigned h = ((unsigned)cx * 73856093u ^ (unsigned)cy * 19349663u ^ (unsigned)cz * 83492791u) & (VS_HASH - 1);
        for (int probe = 0; probe < VS_HASH; ++probe, h = (h + 1) & (VS_HASH - 1)) {       // at most m <= VS_CAP of the 2 VS_CAP slots are taken
            int cur = s_hash[h];
            if (cur == VS_EMPTY) { cur = atomicCAS(&s_hash[h], VS_EMPTY, q); if (cur == VS_EMPTY) break; }
            int ox, oy, oz; cell_of(s_pt[s_lf[cur]], P.inv_leaf, ox, oy, oz);
            if (ox == cx && oy == cy && oz == cz) { atomicMin(&s_hash[h], q); break; }
        }
        s_slot[q] = (unsigned short)h;
    }
    __syncthreads();
    int M2 = 2; while (M2 < m) M2 <<= 1;
    for (int q = tid; q < M2; q += VS_THREADS) s_k32[q] = q < m ? ((unsigned)s_hash[s_slot[q]] << 16) | (unsigned)q : 0xffffffffu;
    __syncthreads();
    lds_bitonic(s_k32, M2, tid);
    int ncell = 0;
    for (int c0 = 0; c0 < m; c0 += VS_THREADS, par ^= 1) {
        const int pos = c0 + tid;
        const unsigned first = pos < m ? s_k32[pos] >> 16 : 0u;
        const bool head = pos < m && (pos == 0 || (s_k32[pos - 1] >> 16) != first);
        int tot;
        const int rk = block_rank(head, tot, s_w[par]);
        if (head) {
            double sx = 0.0, sy = 0.0, sz = 0.0, si = 0.0; int c = 0;
            for (int t = pos; t < m && (s_k32[t] >> 16) == first; ++t, ++c) {
                const float4 p = s_pt[s_lf[s_k32[t] & 0xffffu]];
                sx += (double)p.x; sy += (double)p.y; sz += (double)p.z; si += (double)p.w;
            }
            const double dc = (double)c;
            st_lf[start + ncell + rk] = make_float4((float)(sx / dc), (float)(sy / dc), (float)(sz / dc), (float)(si / dc));
        }
        ncell += tot;
    }
    if (tid == 0) { cnt[RC_LFDS] = ncell; cnt[RC_LFRAW] = m; }
}

__global__ __launch_bounds__(256) void k_scan_gather(ScanP P, const int* __restrict__ table, const int* __restrict__ ring_cnt, const float4* __restrict__ st_sharp,
                                                     const float4* __restrict__ st_less, const float4* __restrict__ st_flat, const float4* __restrict__ st_lf,
                                                     float4* __restrict__ o_sharp, float4* __restrict__ o_less, float4* __restrict__ o_flat, float4* __restrict__ o_lf, int* __restrict__ hdr) {
    __shared__ int s_pre[RC_INTS];
    const int tid = threadIdx.x, r = blockIdx.x;
    if (tid < 5) { int a = 0; for (int q = 0; q < r; ++q) a += ring_cnt[RC_INTS * q + tid]; s_pre[tid] = a; }
    __syncthreads();
    const int* c = ring_cnt + RC_INTS * r;
    const float4* src[4] = {st_sharp + (size_t)r * P.S * P.max_sharp, st_less + (size_t)r * P.S * P.max_less, st_flat + (size_t)r * P.S * P.max_flat, st_lf + table[2 * r]};
    float4* dst[4] = {o_sharp, o_less, o_flat, o_lf};
#pragma unroll
    for (int k = 0; k < 4; ++k) for (int i = tid; i < c[k]; i += 256) dst[k][s_pre[k] + i] = src[k][i];
    if (r + 1 == (int)gridDim.x && tid < 5) hdr[H_SHARP + tid] = s_pre[tid] + c[tid];
}

}  // namespace

struct vscan_ctx : vilhost::Device {                        // d_mem: raw | ring bytes | staging | per-ring counts | result block
    vscan_config cfg;
    ScanP P;
    int max_points = 0;
    size_t cap_sharp = 0, cap_less = 0, cap_flat = 0;      // points: R x S x quota
    float* h_raw = nullptr;                                 // pinned upload image
    char* h_out = nullptr; size_t out_cap = 0;              // pinned mirror of the result block
    size_t o_raw = 0, o_id = 0, o_st_sharp = 0, o_st_less = 0, o_st_flat = 0, o_st_lf = 0, o_cnt = 0, o_out = 0;
    vilhost::Profiler<VSCAN_NUM_KERNELS, VSCAN_NUM_KERNELS + 1> prof;
};

namespace {
// the result block for a scan of n points: header | ring table | labels | cloud | sharp | less | flat | less flat
struct OutLayout { size_t table, labels, cloud, sharp, less, flat, lf, bytes; };
OutLayout out_layout(const vscan_ctx* c, int n) {
    OutLayout L;
    L.table = up16(4 * H_INTS); L.labels = L.table + up16(8 * (size_t)c->P.R); L.cloud = L.labels + up16((size_t)n + 4);
    L.sharp = L.cloud + 16 * (size_t)n; L.less = L.sharp + 16 * c->cap_sharp; L.flat = L.less + 16 * c->cap_less; L.lf = L.flat + 16 * c->cap_flat;
    L.bytes = L.lf + 16 * (size_t)n;
    return L;
}
int set_count(vscan_cloud* o, int count) {
    o->count = count;
    if (!o->xyzi) return VIL_OK;
    if (o->capacity < count) return VIL_ERR_INVALID_ARGUMENT;
    return VIL_OK;
}
}  // namespace

extern "C" {

void vscan_default_config(vscan_config* cfg) {
    if (!cfg) return;
    cfg->num_rings = 16; cfg->lower_bound_deg = -15.0f; cfg->upper_bound_deg = 15.0f;
    cfg->num_scan_subregions = 8; cfg->num_curvature_regions = 5; cfg->surf_curv_th = 1.0f;
    cfg->max_corner_sharp = 3; cfg->max_corner_less_sharp = 30; cfg->max_surf_flat = 4; cfg->less_flat_filter_size = 0.2f; cfg->uneven = 0;
}

int vscan_create(int32_t device, const vscan_config* cfg, int32_t max_points, vscan_ctx** out) {
    if (!out || !cfg || max_points < 1) return VIL_ERR_INVALID_ARGUMENT;
    if (!vilhost::has_device(device)) return VIL_ERR_DEVICE;
    if (cfg->uneven) return VIL_ERR_UNSUPPORTED;
    if (cfg->num_rings < 1 || cfg->num_rings > VSCAN_MAX_RINGS || !(cfg->upper_bound_deg > cfg->lower_bound_deg) || cfg->num_scan_subregions < 1 ||
        cfg->num_scan_subregions > VS_MAX_SUB || cfg->num_curvature_regions < 1 || cfg->num_curvature_regions > 32 || !std::isfinite(cfg->surf_curv_th) ||
        cfg->max_corner_sharp < 0 || cfg->max_corner_sharp > 4096 || cfg->max_corner_less_sharp < 0 || cfg->max_corner_less_sharp > 4096 || cfg->max_surf_flat < 0 ||
        cfg->max_surf_flat > 4096 || !(cfg->less_flat_filter_size > 0.0f) || !std::isfinite(cfg->less_flat_filter_size)) return VIL_ERR_INVALID_ARGUMENT;
    vscan_ctx* c = new vscan_ctx();
    c->cfg = *cfg; c->max_points = max_points;
    ScanP& P = c->P;
    P.R = cfg->num_rings; P.S = cfg->num_scan_subregions; P.C = cfg->num_curvature_regions;
    P.max_sharp = cfg->max_corner_sharp; P.max_less = cfg->max_corner_less_sharp; P.max_flat = cfg->max_surf_flat;
    P.th_hi = cfg->surf_curv_th / 2; P.th_lo = cfg->surf_curv_th / 10; P.inv_leaf = 1.0f / cfg->less_flat_filter_size;
    P.lower = (double)cfg->lower_bound_deg; P.factor = (double)(cfg->num_rings - 1) / ((double)cfg->upper_bound_deg - (double)cfg->lower_bound_deg);
    const size_t RS = (size_t)P.R * P.S, N = (size_t)max_points;
    c->cap_sharp = RS * P.max_sharp; c->cap_less = RS * P.max_less; c->cap_flat = RS * P.max_flat;
    c->out_cap = out_layout(c, max_points).bytes;
    vilhost::Arena a;
    c->o_raw = a.take(16 * N);
    c->o_id = a.take(N + 4);
    c->o_st_sharp = a.take(16 * c->cap_sharp);
    c->o_st_less = a.take(16 * c->cap_less);
    c->o_st_flat = a.take(16 * c->cap_flat);
    c->o_st_lf = a.take(16 * N);
    c->o_cnt = a.take(4 * RC_INTS * (size_t)P.R);
    c->o_out = a.take(c->out_cap);
    hipError_t err = c->open(device, a.bytes);
    if (err == hipSuccess) err = c->pin(&c->h_raw, 16 * N);
    if (err == hipSuccess) err = c->pin(&c->h_out, c->out_cap);
    if (err != hipSuccess) { vscan_destroy(c); VILCHK(err); }
    *out = c;
    return VIL_OK;
}

void vscan_destroy(vscan_ctx* c) {
    if (!c) return;
    c->close(c->prof);
    delete c;
}

int vscan_profile_enable(vscan_ctx* c, int32_t enable) {
    if (!c) return VIL_ERR_INVALID_ARGUMENT;
    VILCHK(c->prof.enable(c->device, enable != 0));
    return VIL_OK;
}
int vscan_profile_read(vscan_ctx* c, int64_t* launches4, double* total_ms4) {
    if (!c || !launches4 || !total_ms4) return VIL_ERR_INVALID_ARGUMENT;
    c->prof.read(launches4, total_ms4);
    return VIL_OK;
}

int vscan_extract(vscan_ctx* c, int32_t n, const float* xyzi, vscan_result* out) {
    if (!c || !out || n < 0 || n > c->max_points || (n && !xyzi)) return VIL_ERR_INVALID_ARGUMENT;
    const ScanP& P = c->P;
    const OutLayout L = out_layout(c, n);
    int* hdr = (int*)c->h_out;
    if (n == 0) memset(c->h_out, 0, L.labels);             // nothing to submit: an empty table, no points
    else {
        VILCHK(hipSetDevice(c->device));
        memcpy(c->h_raw, xyzi, 16 * (size_t)n);
        char* d = c->d_mem; char* dout = d + c->o_out;
        const int npad = (n + 3) & ~3;
        float4* d_raw = (float4*)(d + c->o_raw); unsigned char* d_id = (unsigned char*)(d + c->o_id); int* d_cnt = (int*)(d + c->o_cnt);
        float4* st_sharp = (float4*)(d + c->o_st_sharp); float4* st_less = (float4*)(d + c->o_st_less); float4* st_flat = (float4*)(d + c->o_st_flat); float4* st_lf = (float4*)(d + c->o_st_lf);
        int* d_hdr = (int*)dout; int* d_table = (int*)(dout + L.table); signed char* d_labels = (signed char*)(dout + L.labels); float4* d_cloud = (float4*)(dout + L.cloud);
        VILCHK(hipMemcpyAsync(d_raw, c->h_raw, 16 * (size_t)n, hipMemcpyHostToDevice, c->stream));
        VILCHK(c->prof.mark(0, c->stream));
        hipLaunchKernelGGL(k_scan_ring_id, dim3((npad + 255) / 256), dim3(256), 0, c->stream, n, npad, d_raw, d_id, P);
        VILCHK(c->prof.mark(1, c->stream));
        hipLaunchKernelGGL(k_scan_ring_sort, dim3(P.R), dim3(VS_THREADS), 0, c->stream, npad, d_raw, d_id, d_table, d_cloud, d_hdr);
        VILCHK(c->prof.mark(2, c->stream));
        hipLaunchKernelGGL(k_scan_features, dim3(P.R), dim3(VS_THREADS), 0, c->stream, P, d_table, d_cloud, d_labels, st_sharp, st_less, st_flat, st_lf, d_cnt, d_hdr);
        VILCHK(c->prof.mark(3, c->stream));
        hipLaunchKernelGGL(k_scan_gather, dim3(P.R), dim3(256), 0, c->stream, P, d_table, d_cnt, st_sharp, st_less, st_flat, st_lf, (float4*)(dout + L.sharp), (float4*)(dout + L.less),
                           (float4*)(dout + L.flat), (float4*)(dout + L.lf), d_hdr);
        VILCHK(c->prof.mark(4, c->stream));
        VILCHK(hipMemcpyAsync(c->h_out, dout, L.bytes, hipMemcpyDeviceToHost, c->stream));
        VILCHK(hipStreamSynchronize(c->stream));
        VILCHK(hipGetLastError());
        for (int k = 0; k < VSCAN_NUM_KERNELS; ++k) c->prof.span(k, k, k + 1);
    }
    const int nvalid = hdr[H_NVALID];
    out->num_rings = P.R; out->n_less_flat_raw = hdr[H_LFRAW];
    int bad = 0;
    bad |= set_count(&out->cloud, nvalid);
    bad |= set_count(&out->corner_sharp, hdr[H_SHARP]);
    bad |= set_count(&out->corner_less_sharp, hdr[H_LESS]);
    bad |= set_count(&out->surf_flat, hdr[H_FLAT]);
    bad |= set_count(&out->surf_less_flat, hdr[H_LFDS]);
    if (out->ring_table && out->ring_capacity < P.R) bad = 1;
    if (out->labels && out->label_capacity < nvalid) bad = 1;
    if (hdr[H_OVER]) return VIL_ERR_UNSUPPORTED;
    if (bad) return VIL_ERR_INVALID_ARGUMENT;
    if (out->ring_table) memcpy(out->ring_table, c->h_out + L.table, 8 * (size_t)P.R);
    if (out->labels && nvalid) memcpy(out->labels, c->h_out + L.labels, (size_t)nvalid);
    const struct { vscan_cloud* o; size_t off; } cl[5] = {{&out->cloud, L.cloud}, {&out->corner_sharp, L.sharp}, {&out->corner_less_sharp, L.less}, {&out->surf_flat, L.flat}, {&out->surf_less_flat, L.lf}};
    for (const auto& k : cl) if (k.o->xyzi && k.o->count) memcpy(k.o->xyzi, c->h_out + k.off, 16 * (size_t)k.o->count);
    return VIL_OK;
}

}  // extern "C"
