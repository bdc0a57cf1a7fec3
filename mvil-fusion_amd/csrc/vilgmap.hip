// vilgmap.hip -- the global map of lidar_mapping resident on gfx950 behind include/vilgmap.h (the steps are numbered as in the header).
//
// Resident: the map points, the voxel table (packed 63-bit keys + the smallest point index per voxel), the keyed scans, a scratch table for
// the reference's thinning, one mark per map point.  An insert, whatever its source (host points, a stored scan, all stored scans of a
// rebuild), is a list of segments {transform, source offset, first input index} and ONE submission:
//   k_gmap_wipe     rebuild only: empties the table (returns on the flag, so a refused rebuild keeps the old map)
//   k_gmap_xform    steps 1 and 2 per input point: the point's segment by bisection, the transformed point, its voxel key; a voxel index
//                   outside 2^20 raises the flag in rec[0]
//   k_gmap_claim    step 3: the key's slot (bounded linear probing, atomicCAS on an empty slot), atomicMin(val[slot], n_map + i)
//   k_gmap_survive  survivor flags (val[slot] == n_map + i) and the survivors per workgroup
//   k_gmap_scan     exclusive scan of those counts by one workgroup; rec[1] = the new n_map
//   k_gmap_append   ordered compaction: survivor -> map[n_map + offset + rank]; val[slot] becomes that final index, so that every value in
//                   the table stays below the global indices of all later inputs
// and one read-back of rec.  vgmap_reference over the uniform grid of vil_knn.hpp (rebuilt lazily when the map has changed):
//   k_gmap_radius   step 5, a WAVE per query point: the (up to 4 x 4 x 4) cells that meet the query's box are looked up by the lanes, their
//                   points read 64 at a time; a point in range gets mark[j] = epoch (a plain store of one value)
//   k_gmap_thin     marked points claim their reference voxel in the scratch table (atomicMin of j); k_gmap_pick flags and counts,
//                   k_gmap_scan, k_gmap_emit compacts in ascending j (step 7 applied), k_gmap_unclaim empties the slots that were used
//   k_gmap_knn      step 6, a wave per query point through knn_wave_query<true>; k_gmap_scan over the per-query counts, k_gmap_emit
// Nothing that feeds a compared number may be contracted into an fma:
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>

#include "../../include/vilgmap.h"
#include "vil_host.hpp"
#include "vil_knn.hpp"

#define VG_BLK 256                   // threads per workgroup of the per-point kernels; the compaction's partition
#define VG_QPB 4                     // queries (waves) per workgroup of the search kernels
#define VG_SCAN 1024                 // threads of k_gmap_scan

namespace {

using namespace vknn;

enum { K_XFORM = 0, K_CLAIM, K_SURVIVE, K_SCAN, K_APPEND, K_WIPE, K_GRID, K_RADIUS, K_THIN, K_PICK, K_EMIT, K_UNCLAIM, K_KNN };
enum { E_MAX = 10 };

struct Seg { double m[12]; int src, first; };           // first three rows of T; offset (points) into the source cloud; first input index
struct Tab { long long* keys; int* val; unsigned mask; };
struct Vox { double ox, oy, oz, res; };

// step 1: the point promoted to double, unfused, rounded to float.  Contraction is off where the operations are written.
__device__ __forceinline__ void transform_point(const double* __restrict__ m, float fx, float fy, float fz, float& qx, float& qy, float& qz) {
#pragma clang fp contract(off)
    const double x = (double)fx, y = (double)fy, z = (double)fz;
    qx = (float)(((m[0] * x + m[1] * y) + m[2] * z) + m[3]);
    qy = (float)(((m[4] * x + m[5] * y) + m[6] * z) + m[7]);
    qz = (float)(((m[8] * x + m[9] * y) + m[10] * z) + m[11]);
}

// step 2; -1: a voxel index outside 2^20
__device__ __forceinline__ long long voxel_key(const Vox& v, float px, float py, float pz) {
#pragma clang fp contract(off)
    const double cx = floor(((double)px - v.ox) / v.res), cy = floor(((double)py - v.oy) / v.res), cz = floor(((double)pz - v.oz) / v.res);
    const double L = (double)VGMAP_VOXEL_LIMIT;
    if (!(fabs(cx) < L && fabs(cy) < L && fabs(cz) < L)) return -1;
    return (((long long)cx + VGMAP_VOXEL_LIMIT) << 42) | (((long long)cy + VGMAP_VOXEL_LIMIT) << 21) | ((long long)cz + VGMAP_VOXEL_LIMIT);
}

// the key's slot, claimed when the key is new.  At most mask + 1 probes; -1 when the table holds mask + 1 other keys (it never does: the
// table has twice as many slots as the map has points).  keys only ever change from -1 to a key, so a stale read costs one atomicCAS.
__device__ __forceinline__ int tab_slot(const Tab& t, long long key) {
    unsigned h = hash_key(key) & t.mask;
    for (unsigned p = 0; p <= t.mask; ++p, h = (h + 1) & t.mask) {
        long long k = t.keys[h];
        if (k == key) return (int)h;
        if (k < 0) {
            k = (long long)atomicCAS((unsigned long long*)(t.keys + h), (unsigned long long)-1LL, (unsigned long long)key);
            if (k < 0 || k == key) return (int)h;
        }
    }
    return -1;
}

// ordered compaction, first half: the workgroup's number of kept items
__device__ __forceinline__ void block_count(bool ok, int* __restrict__ blk) {
    __shared__ int s_cnt;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    const unsigned long long b = __ballot(ok);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&s_cnt, __popcll(b));
    __syncthreads();
    if (threadIdx.x == 0) blk[blockIdx.x] = s_cnt;
}
// second half: a kept item's position = the workgroups before it (off, from k_gmap_scan) + the waves before it + the lanes before it
__device__ __forceinline__ int block_rank(bool ok, const int* __restrict__ off) {
    __shared__ int s_w[VG_BLK / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long b = __ballot(ok);
    if (lane == 0) s_w[w] = __popcll(b);
    __syncthreads();
    int pos = off[blockIdx.x] + __popcll(b & ((1ull << lane) - 1ull));
    for (int v = 0; v < w; ++v) pos += s_w[v];
    return pos;
}

__global__ __launch_bounds__(VG_BLK) void k_gmap_wipe(Tab t, const int* __restrict__ rec) {
    if (rec[0]) return;
    const size_t e = (size_t)blockIdx.x * VG_BLK + threadIdx.x;
    if (e <= t.mask) { t.keys[e] = -1; t.val[e] = INT_MAX; }
}

__global__ __launch_bounds__(VG_BLK) void k_gmap_xform(int n, int nseg, const Seg* __restrict__ seg, const float* __restrict__ src, Vox v, float* __restrict__ q,
                                                       long long* __restrict__ key, int* __restrict__ rec) {
    const int i = blockIdx.x * VG_BLK + threadIdx.x;
    if (i >= n) return;
    int lo = 0, hi = nseg - 1;                              // the last segment whose first index is <= i
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (seg[mid].first <= i) lo = mid; else hi = mid - 1; }
    const Seg& s = seg[lo];
    const float* p = src + 3 * ((size_t)s.src + (size_t)(i - s.first));
    float qx, qy, qz;
    transform_point(s.m, p[0], p[1], p[2], qx, qy, qz);
    q[3 * (size_t)i] = qx; q[3 * (size_t)i + 1] = qy; q[3 * (size_t)i + 2] = qz;
    if (v.res > 0.0) {
        const long long k = voxel_key(v, qx, qy, qz);
        key[i] = k;
        if (k < 0) rec[0] = 1;
    }
}

__global__ __launch_bounds__(VG_BLK) void k_gmap_claim(int n, int n_map, Tab t, const long long* __restrict__ key, int* __restrict__ slot, int* __restrict__ rec) {
    if (rec[0]) return;
    const int i = blockIdx.x * VG_BLK + threadIdx.x;
    if (i >= n) return;
    const int s = tab_slot(t, key[i]);
    slot[i] = s;
    if (s >= 0) atomicMin(t.val + s, n_map + i); else rec[2] = 1;
}

// thin = false (map_resolution <= 0): every point survives and no table is kept
__global__ __launch_bounds__(VG_BLK) void k_gmap_survive(int n, int n_map, bool thin, Tab t, const int* __restrict__ slot, int* __restrict__ blk, const int* __restrict__ rec) {
    if (rec[0]) return;
    const int i = blockIdx.x * VG_BLK + threadIdx.x;
    bool ok = i < n;
    if (ok && thin) { const int s = slot[i]; ok = s >= 0 && t.val[s] == n_map + i; }
    block_count(ok, blk);
}

// off = exclusive scan of cnt[0 .. m); rec[1] = base + the total.  One workgroup, VG_SCAN items per round, a carry between the rounds.
__global__ __launch_bounds__(VG_SCAN) void k_gmap_scan(int m, const int* __restrict__ cnt, int* __restrict__ off, int base, int* __restrict__ rec) {
    __shared__ int s_w[VG_SCAN / 64];
    __shared__ int s_carry;
    if (rec[0]) return;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    if (t == 0) s_carry = 0;
    __syncthreads();
    for (int b0 = 0; b0 < m; b0 += VG_SCAN) {
        const int e = b0 + t, c = e < m ? cnt[e] : 0;
        int incl = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(incl, o, 64); incl += lane >= o ? u : 0; }
        if (lane == 63) s_w[w] = incl;
        __syncthreads();
        int before = s_carry;
        for (int u = 0; u < w; ++u) before += s_w[u];
        if (e < m) off[e] = before + incl - c;
        __syncthreads();
        if (t == VG_SCAN - 1) s_carry = before + incl;
        __syncthreads();
    }
    if (t == 0) rec[1] = base + s_carry;
}

__global__ __launch_bounds__(VG_BLK) void k_gmap_append(int n, int n_map, bool thin, Tab t, const int* __restrict__ slot, const int* __restrict__ off, const float* __restrict__ q,
                                                        float* __restrict__ map, int max_map, const int* __restrict__ rec) {
    if (rec[0]) return;
    const int i = blockIdx.x * VG_BLK + threadIdx.x;
    bool ok = i < n;
    int s = -1;
    if (ok && thin) { s = slot[i]; ok = s >= 0 && t.val[s] == n_map + i; }
    const int pos = n_map + block_rank(ok, off);
    // A survivor's rewritten val is pos <= n_map + i, below the global index of every other point of its voxel: whether such a point reads
    // val before or after the rewrite, it does not find its own index there.
    if (ok && pos < max_map) {                              // pos <= n_map + i < max_map: the host checked n_map + n
        map[3 * (size_t)pos] = q[3 * (size_t)i]; map[3 * (size_t)pos + 1] = q[3 * (size_t)i + 1]; map[3 * (size_t)pos + 2] = q[3 * (size_t)i + 2];
        if (thin) t.val[s] = pos;
    }
}

// step 5.  The grid's cell edge h is a power of two not below the radius, so cell indices are exact; a point with float d2 <= r2 differs from
// the query by at most radius * (1 + 1e-6) per axis, and the box of half-width pad = radius * (1 + 1e-5) around the query meets at most
// four cells per axis.
__global__ __launch_bounds__(64 * VG_QPB) void k_gmap_radius(int nq, const float* __restrict__ src, const Seg* __restrict__ seg, float r2, double pad, GridTab G, const int* __restrict__ order,
                                                             const float* __restrict__ cxyz, int epoch, int* __restrict__ mark) {
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int i = blockIdx.x * VG_QPB + wave;
    if (i >= nq) return;                                    // wave-uniform
    float qx, qy, qz;
    transform_point(seg[0].m, src[3 * (size_t)i], src[3 * (size_t)i + 1], src[3 * (size_t)i + 2], qx, qy, qz);
    const double h = (double)G.h;
    const int x0 = (int)floor(((double)qx - pad) / h), y0 = (int)floor(((double)qy - pad) / h), z0 = (int)floor(((double)qz - pad) / h);
    const int x1 = (int)floor(((double)qx + pad) / h), y1 = (int)floor(((double)qy + pad) / h), z1 = (int)floor(((double)qz + pad) / h);
    const int cx = x0 + (lane & 3), cy = y0 + ((lane >> 2) & 3), cz = z0 + (lane >> 4);
    int b = 0, cnt = 0;
    if (cx <= x1 && cy <= y1 && cz <= z1) {
        const int s = grid_slot(G, pack_key(cx, cy, cz), false);
        if (s >= 0) { b = G.start[s]; cnt = G.cnt[s]; }
    }
    unsigned long long live = __ballot(cnt > 0);
    while (live) {
        const int c = __builtin_ctzll(live);
        live &= live - 1;
        const int cb = __builtin_amdgcn_readlane(b, c), cc = __builtin_amdgcn_readlane(cnt, c);
        for (int t = lane; t < cc; t += 64) {
            const int pos = cb + t;
            if (sqdist_strict(qx, qy, qz, cxyz[3 * (size_t)pos], cxyz[3 * (size_t)pos + 1], cxyz[3 * (size_t)pos + 2]) <= r2) mark[order[pos]] = epoch;
        }
    }
}

// the marked points claim their reference voxel in the scratch table.  First kernel of the thinning: a voxel index outside 2^20 raises the flag.
__global__ __launch_bounds__(VG_BLK) void k_gmap_thin(int n_map, const float* __restrict__ map, const int* __restrict__ mark, int epoch, Vox v, Tab t, int* __restrict__ slot,
                                                      int* __restrict__ rec) {
    const int j = blockIdx.x * VG_BLK + threadIdx.x;
    if (j >= n_map || mark[j] != epoch) return;
    const long long k = voxel_key(v, map[3 * (size_t)j], map[3 * (size_t)j + 1], map[3 * (size_t)j + 2]);
    int s = -1;
    if (k < 0) rec[0] = 1; else s = tab_slot(t, k);
    slot[j] = s;
    if (s >= 0) atomicMin(t.val + s, j); else if (k >= 0) rec[2] = 1;
}

__global__ __launch_bounds__(VG_BLK) void k_gmap_pick(int n_map, const int* __restrict__ mark, int epoch, bool thin, Tab t, const int* __restrict__ slot, int* __restrict__ blk,
                                                      const int* __restrict__ rec) {
    if (rec[0]) return;
    const int j = blockIdx.x * VG_BLK + threadIdx.x;
    bool ok = j < n_map && mark[j] == epoch;
    if (ok && thin) { const int s = slot[j]; ok = s >= 0 && t.val[s] == j; }
    block_count(ok, blk);
}

// radius mode (knn_j = NULL): item = map point j, kept as in k_gmap_pick, at off[workgroup] + rank.  kNN mode: item = (query, place) = (e / k, e % k),
// kept when place < cnt[query], at off[query] + place.  Step 7 on the way out; nothing is written past max_ref.
__global__ __launch_bounds__(VG_BLK) void k_gmap_emit(int n_items, const float* __restrict__ map, const int* __restrict__ mark, int epoch, bool thin, Tab t, const int* __restrict__ slot,
                                                      const int* __restrict__ off, const int* __restrict__ knn_j, const int* __restrict__ knn_cnt, int k, const Seg* __restrict__ seg,
                                                      bool has_out, int max_ref, float* __restrict__ ref_xyz, int* __restrict__ ref_idx, const int* __restrict__ rec) {
    if (rec[0]) return;
    const int e = blockIdx.x * VG_BLK + threadIdx.x;
    int j = e, pos;
    bool ok;
    if (knn_j) {
        const int qi = e / k, place = e - qi * k;
        ok = e < n_items && place < knn_cnt[qi];
        pos = ok ? off[qi] + place : 0;
        if (ok) j = knn_j[e];
    } else {
        ok = e < n_items && mark[e] == epoch;
        if (ok && thin) { const int s = slot[e]; ok = s >= 0 && t.val[s] == e; }
        pos = block_rank(ok, off);
    }
    if (!ok || pos >= max_ref) return;
    float x = map[3 * (size_t)j], y = map[3 * (size_t)j + 1], z = map[3 * (size_t)j + 2];
    if (has_out) transform_point(seg[1].m, x, y, z, x, y, z);
    ref_xyz[3 * (size_t)pos] = x; ref_xyz[3 * (size_t)pos + 1] = y; ref_xyz[3 * (size_t)pos + 2] = z;
    ref_idx[pos] = j;
}

// the scratch table goes back to empty: only the slots this query used are touched.  Runs whatever the flag says.
__global__ __launch_bounds__(VG_BLK) void k_gmap_unclaim(int n_map, const int* __restrict__ mark, int epoch, Tab t, const int* __restrict__ slot) {
    const int j = blockIdx.x * VG_BLK + threadIdx.x;
    if (j >= n_map || mark[j] != epoch) return;
    const int s = slot[j];
    if (s >= 0) { t.keys[s] = -1; t.val[s] = INT_MAX; }    // several points of a voxel store the same two values
}

// step 6.  reject_d2 is a little above max_dist: a query whose k-th best is not below it stops as soon as everything unvisited is farther.
__global__ __launch_bounds__(64 * VG_QPB) void k_gmap_knn(int nq, const float* __restrict__ src, const Seg* __restrict__ seg, int k, float max_dist, float reject_d2, int n_map, GridTab G,
                                                          const int* __restrict__ order, const float* __restrict__ cxyz, int* __restrict__ knn_j, int* __restrict__ knn_cnt) {
    __shared__ int wl_all[VG_QPB * KNN_WL_CAP];
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int i = blockIdx.x * VG_QPB + wave;
    if (i >= nq) return;                                    // wave-uniform; knn_wave_query has no workgroup barrier
    float qx, qy, qz;
    transform_point(seg[0].m, src[3 * (size_t)i], src[3 * (size_t)i + 1], src[3 * (size_t)i + 2], qx, qy, qz);
    unsigned long long best;
    knn_wave_query<true>(best, qx, qy, qz, k, n_map, G, order, cxyz, wl_all + wave * KNN_WL_CAP, reject_d2, k);
    const bool in = lane < k && best != ~0ull && knn_key_d(best) <= max_dist;      // the list is sorted: the lanes in range are a prefix
    if (in) knn_j[(size_t)i * k + lane] = (int)(unsigned)best;
    const unsigned long long b = __ballot(in);
    if (lane == 0) knn_cnt[i] = __popcll(b);
}

bool all_finite(const float* xyz, size_t count) {
    for (size_t i = 0; i < count; ++i) if (!std::isfinite(xyz[i])) return false;
    return true;
}
bool all_finite(const double* v, size_t count) {
    for (size_t i = 0; i < count; ++i) if (!std::isfinite(v[i])) return false;
    return true;
}

struct Scan { int off, n; };

}  // namespace

struct vgmap_ctx : vilhost::Device {         // d_mem: map | table | scratch table | keyed scans | input | q | keys | slots | marks | counts | offsets | knn | segments | reference | rec
    vgmap_config cfg;
    int n_map = 0, n_keyed = 0, epoch = 0, max_in = 0, max_blk = 0;
    unsigned slots = 0;
    std::map<int32_t, Scan> scans;
    vknn::GridBuild gb; float grid_h = 0.f; bool grid_valid = false;
    float* h_in = nullptr; Seg* h_seg = nullptr; char* h_out = nullptr; int* h_rec = nullptr;      // pinned
    size_t o_map = 0, o_keys = 0, o_val = 0, o_skeys = 0, o_sval = 0, o_keyed = 0, o_in = 0, o_q = 0, o_key = 0, o_slot = 0, o_mslot = 0, o_mark = 0, o_blk = 0, o_off = 0, o_knnj = 0,
           o_knnc = 0, o_seg = 0, o_rxyz = 0, o_ridx = 0, o_rec = 0;
    vilhost::Profiler<VGMAP_NUM_KERNELS, E_MAX> prof;

    template <class T> T* at(size_t off) { return (T*)(d_mem + off); }
    Tab tab() { return Tab{at<long long>(o_keys), at<int>(o_val), slots - 1}; }
    Tab scratch() { return Tab{at<long long>(o_skeys), at<int>(o_sval), slots - 1}; }
    Vox vox(float res) const { return Vox{cfg.origin[0], cfg.origin[1], cfg.origin[2], (double)res}; }
};

namespace {

inline int nblk(int n) { return (n + VG_BLK - 1) / VG_BLK; }

int wipe_table(vgmap_ctx* c, Tab t) {
    hipLaunchKernelGGL(k_gmap_wipe, dim3((unsigned)((t.mask + (size_t)VG_BLK) / VG_BLK)), dim3(VG_BLK), 0, c->stream, t, c->at<int>(c->o_rec));
    return VIL_OK;
}

// steps 1 - 3 of n input points described by h_seg[0 .. nseg) over the device cloud src; rebuild: from an empty map.  One submission.
int submit_insert(vgmap_ctx* c, int n, int nseg, const float* src, bool rebuild) {
    const int base = rebuild ? 0 : c->n_map, nb = nblk(n);
    const bool thin = c->cfg.map_resolution > 0.f;
    int* rec = c->at<int>(c->o_rec);
    Tab t = c->tab();
    VILCHK(hipMemsetAsync(rec, 0, 16, c->stream));
    VILCHK(hipMemcpyAsync(c->d_mem + c->o_seg, c->h_seg, sizeof(Seg) * (size_t)nseg, hipMemcpyHostToDevice, c->stream));
    VILCHK(c->prof.mark(0, c->stream));
    hipLaunchKernelGGL(k_gmap_xform, dim3(nb), dim3(VG_BLK), 0, c->stream, n, nseg, c->at<Seg>(c->o_seg), src, c->vox(c->cfg.map_resolution), c->at<float>(c->o_q), c->at<long long>(c->o_key), rec);
    VILCHK(c->prof.mark(1, c->stream));
    if (rebuild && thin) wipe_table(c, t);
    VILCHK(c->prof.mark(2, c->stream));
    if (thin) hipLaunchKernelGGL(k_gmap_claim, dim3(nb), dim3(VG_BLK), 0, c->stream, n, base, t, c->at<long long>(c->o_key), c->at<int>(c->o_slot), rec);
    VILCHK(c->prof.mark(3, c->stream));
    hipLaunchKernelGGL(k_gmap_survive, dim3(nb), dim3(VG_BLK), 0, c->stream, n, base, thin, t, c->at<int>(c->o_slot), c->at<int>(c->o_blk), rec);
    VILCHK(c->prof.mark(4, c->stream));
    hipLaunchKernelGGL(k_gmap_scan, dim3(1), dim3(VG_SCAN), 0, c->stream, nb, c->at<int>(c->o_blk), c->at<int>(c->o_off), base, rec);
    VILCHK(c->prof.mark(5, c->stream));
    hipLaunchKernelGGL(k_gmap_append, dim3(nb), dim3(VG_BLK), 0, c->stream, n, base, thin, t, c->at<int>(c->o_slot), c->at<int>(c->o_off), c->at<float>(c->o_q), c->at<float>(c->o_map),
                       c->cfg.max_map_points, rec);
    VILCHK(c->prof.mark(6, c->stream));
    VILCHK(hipMemcpyAsync(c->h_rec, rec, 16, hipMemcpyDeviceToHost, c->stream));
    VILCHK(hipStreamSynchronize(c->stream));
    VILCHK(hipGetLastError());
    c->prof.span(K_XFORM, 0, 1);
    if (rebuild && thin) c->prof.span(K_WIPE, 1, 2);
    if (thin) c->prof.span(K_CLAIM, 2, 3);
    c->prof.span(K_SURVIVE, 3, 4); c->prof.span(K_SCAN, 4, 5); c->prof.span(K_APPEND, 5, 6);
    if (c->h_rec[0]) return VIL_ERR_INVALID_ARGUMENT;       // a voxel index outside 2^20: nothing after k_gmap_xform ran
    if (c->h_rec[2]) return VIL_ERR_CAPACITY;               // unreachable: the table has room for twice the map
    c->n_map = c->h_rec[1];
    c->grid_valid = false;
    return VIL_OK;
}

void set_seg(Seg& s, const double* T16, int src, int first) { memcpy(s.m, T16, sizeof s.m); s.src = src; s.first = first; }

}  // namespace

extern "C" {

void vgmap_default_config(vgmap_config* g) {
    if (!g) return;
    g->max_map_points = 1 << 22; g->max_scan_points = 1 << 17; g->max_keys = 4096; g->max_keyed_points = 1 << 24; g->max_ref_points = 1 << 18;
    g->map_resolution = 0.05f; g->origin[0] = g->origin[1] = g->origin[2] = 0.0;
}

void vgmap_default_ref_options(vgmap_ref_options* o) {
    if (!o) return;
    o->mode = VGMAP_REF_RADIUS; o->k = 5; o->radius = 0.5; o->ref_resolution = 0.3f; o->max_dist = 1.5f;
}

int vgmap_create(int32_t device, const vgmap_config* g, vgmap_ctx** out) {
    if (!out || !g || g->max_map_points <= 0 || g->max_scan_points <= 0 || g->max_keys <= 0 || g->max_keyed_points <= 0 || g->max_ref_points <= 0 ||
        g->max_map_points > (1 << 29) || g->max_scan_points > (1 << 24) || !std::isfinite(g->map_resolution) || !all_finite(g->origin, 3))
        return VIL_ERR_INVALID_ARGUMENT;
    vgmap_ctx* c = new vgmap_ctx();
    c->cfg = *g;
    c->slots = 1024; while (c->slots < 2u * (unsigned)g->max_map_points) c->slots <<= 1;
    c->max_in = g->max_map_points > g->max_scan_points ? g->max_map_points : g->max_scan_points;      // a rebuild's input is at most max_map_points
    c->max_blk = nblk(c->max_in);
    const size_t M = (size_t)g->max_map_points, S = c->slots, W = (size_t)c->max_in, Q = (size_t)g->max_scan_points, R = (size_t)g->max_ref_points;
    const size_t cnts = (size_t)c->max_blk > Q ? (size_t)c->max_blk : Q;                               // k_gmap_scan's input: workgroups, or queries
    vilhost::Arena a;
    c->o_map = a.take(12 * M);
    c->o_keys = a.take(8 * S); c->o_val = a.take(4 * S);
    c->o_skeys = a.take(8 * S); c->o_sval = a.take(4 * S);
    c->o_keyed = a.take(12 * (size_t)g->max_keyed_points);
    c->o_in = a.take(12 * Q);
    c->o_q = a.take(12 * W); c->o_key = a.take(8 * W); c->o_slot = a.take(4 * W);
    c->o_mslot = a.take(4 * M); c->o_mark = a.take(4 * M);
    c->o_blk = a.take(4 * cnts); c->o_off = a.take(4 * cnts);
    c->o_knnj = a.take(4 * Q * VGMAP_MAX_K); c->o_knnc = a.take(4 * Q);
    c->o_seg = a.take(sizeof(Seg) * ((size_t)g->max_keys + 2));
    c->o_rxyz = a.take(12 * R); c->o_ridx = a.take(4 * R);
    c->o_rec = a.take(16);
    hipError_t err = c->open(device, a.bytes);
    if (err == hipSuccess) err = c->pin(&c->h_in, 12 * Q);
    if (err == hipSuccess) err = c->pin(&c->h_seg, sizeof(Seg) * ((size_t)g->max_keys + 2));
    if (err == hipSuccess) err = c->pin(&c->h_out, 16 * R);
    if (err == hipSuccess) err = c->pin(&c->h_rec, 16);
    if (err == hipSuccess) err = hipMemsetAsync(c->d_mem + c->o_keys, 0xFF, 8 * S, c->stream);        // every key = -1 (empty)
    if (err == hipSuccess) err = hipMemsetAsync(c->d_mem + c->o_skeys, 0xFF, 8 * S, c->stream);
    if (err == hipSuccess) err = hipMemsetAsync(c->d_mem + c->o_mark, 0, 4 * M, c->stream);           // epoch 0 marks nothing: the first query has epoch 1
    if (err == hipSuccess) err = hipMemsetAsync(c->d_mem + c->o_rec, 0, 16, c->stream);
    if (err == hipSuccess) {                                                                           // every val = INT_MAX
        wipe_table(c, c->tab()); wipe_table(c, c->scratch());
        err = hipStreamSynchronize(c->stream);
    }
    if (err == hipSuccess) err = hipGetLastError();
    if (err != hipSuccess) { vgmap_destroy(c); VILCHK(err); }
    *out = c;
    return VIL_OK;
}

void vgmap_destroy(vgmap_ctx* c) {
    if (!c) return;
    c->close(c->prof);
    delete c;
}

int vgmap_profile_enable(vgmap_ctx* c, int32_t enable) {
    if (!c) return VIL_ERR_INVALID_ARGUMENT;
    VILCHK(c->prof.enable(c->device, enable != 0));
    return VIL_OK;
}
int vgmap_profile_read(vgmap_ctx* c, int64_t* launches13, double* total_ms13) {
    if (!c || !launches13 || !total_ms13) return VIL_ERR_INVALID_ARGUMENT;
    c->prof.read(launches13, total_ms13);
    return VIL_OK;
}

int vgmap_add_scan(vgmap_ctx* c, int32_t key, int32_t n, const float* xyz) {
    if (!c || !xyz || n < 1 || n > c->cfg.max_scan_points || c->scans.count(key)) return VIL_ERR_INVALID_ARGUMENT;
    if (!all_finite(xyz, 3 * (size_t)n)) return VIL_ERR_NON_FINITE;
    if ((int)c->scans.size() >= c->cfg.max_keys || (long long)c->n_keyed + n > c->cfg.max_keyed_points) return VIL_ERR_CAPACITY;
    VILCHK(hipSetDevice(c->device));
    memcpy(c->h_in, xyz, 12 * (size_t)n);
    VILCHK(hipMemcpyAsync(c->d_mem + c->o_keyed + 12 * (size_t)c->n_keyed, c->h_in, 12 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    VILCHK(hipStreamSynchronize(c->stream));                 // the pinned buffer is free again
    c->scans[key] = Scan{c->n_keyed, n};
    c->n_keyed += n;
    return VIL_OK;
}

int vgmap_insert(vgmap_ctx* c, int32_t n, const float* xyz, const double* T16) {
    if (!c || !xyz || !T16 || n < 1 || n > c->cfg.max_scan_points) return VIL_ERR_INVALID_ARGUMENT;
    if (!all_finite(xyz, 3 * (size_t)n) || !all_finite(T16, 12)) return VIL_ERR_NON_FINITE;
    if ((long long)c->n_map + n > c->cfg.max_map_points) return VIL_ERR_CAPACITY;
    VILCHK(hipSetDevice(c->device));
    memcpy(c->h_in, xyz, 12 * (size_t)n);
    VILCHK(hipMemcpyAsync(c->d_mem + c->o_in, c->h_in, 12 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    set_seg(c->h_seg[0], T16, 0, 0);
    return submit_insert(c, n, 1, c->at<float>(c->o_in), false);
}

int vgmap_insert_key(vgmap_ctx* c, int32_t key, const double* T16) {
    if (!c || !T16) return VIL_ERR_INVALID_ARGUMENT;
    const auto it = c->scans.find(key);
    if (it == c->scans.end()) return VIL_ERR_INVALID_ARGUMENT;
    if (!all_finite(T16, 12)) return VIL_ERR_NON_FINITE;
    if ((long long)c->n_map + it->second.n > c->cfg.max_map_points) return VIL_ERR_CAPACITY;
    VILCHK(hipSetDevice(c->device));
    set_seg(c->h_seg[0], T16, it->second.off, 0);
    return submit_insert(c, it->second.n, 1, c->at<float>(c->o_keyed), false);
}

int vgmap_rebuild(vgmap_ctx* c, int32_t n_keys, const int32_t* keys, const double* T16s) {
    if (!c || !keys || !T16s || n_keys < 1 || n_keys > c->cfg.max_keys) return VIL_ERR_INVALID_ARGUMENT;
    long long total = 0;
    for (int k = 0; k < n_keys; ++k) {
        const auto it = c->scans.find(keys[k]);
        if (it == c->scans.end() || (k && keys[k] <= keys[k - 1])) return VIL_ERR_INVALID_ARGUMENT;
        total += it->second.n;
    }
    for (int k = 0; k < n_keys; ++k) if (!all_finite(T16s + 16 * (size_t)k, 12)) return VIL_ERR_NON_FINITE;
    if (total > c->cfg.max_map_points) return VIL_ERR_CAPACITY;
    VILCHK(hipSetDevice(c->device));
    int first = 0;
    for (int k = 0; k < n_keys; ++k) { const Scan& s = c->scans[keys[k]]; set_seg(c->h_seg[k], T16s + 16 * (size_t)k, s.off, first); first += s.n; }
    return submit_insert(c, (int)total, n_keys, c->at<float>(c->o_keyed), true);
}

int vgmap_clear(vgmap_ctx* c) {
    if (!c) return VIL_ERR_INVALID_ARGUMENT;
    VILCHK(hipSetDevice(c->device));
    VILCHK(hipMemsetAsync(c->d_mem + c->o_rec, 0, 16, c->stream));
    wipe_table(c, c->tab());
    VILCHK(hipStreamSynchronize(c->stream));
    VILCHK(hipGetLastError());
    c->n_map = 0; c->grid_valid = false;
    return VIL_OK;
}

int vgmap_size(vgmap_ctx* c, int32_t* n_map, int32_t* n_keys, int32_t* n_keyed_points) {
    if (!c) return VIL_ERR_INVALID_ARGUMENT;
    if (n_map) *n_map = c->n_map;
    if (n_keys) *n_keys = (int32_t)c->scans.size();
    if (n_keyed_points) *n_keyed_points = c->n_keyed;
    return VIL_OK;
}

int vgmap_get_points(vgmap_ctx* c, int32_t first, int32_t n, float* xyz) {
    if (!c || !xyz || first < 0 || n < 1 || (long long)first + n > c->n_map) return VIL_ERR_INVALID_ARGUMENT;
    VILCHK(hipSetDevice(c->device));
    VILCHK(hipMemcpyAsync(xyz, c->d_mem + c->o_map + 12 * (size_t)first, 12 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    VILCHK(hipStreamSynchronize(c->stream));
    return VIL_OK;
}

int vgmap_reference(vgmap_ctx* c, int32_t n, const float* xyz, const double* T16, const vgmap_ref_options* o, const double* T_out16, int32_t* n_ref, float* ref_xyz, int32_t* ref_idx) {
    if (!c || !xyz || !T16 || !o || !n_ref || !ref_xyz || n < 1 || n > c->cfg.max_scan_points) return VIL_ERR_INVALID_ARGUMENT;
    const bool knn = o->mode == VGMAP_REF_KNN;
    if (!knn && o->mode != VGMAP_REF_RADIUS) return VIL_ERR_INVALID_ARGUMENT;
    if (knn ? (o->k < 1 || o->k > VGMAP_MAX_K || std::isnan(o->max_dist)) : (!(o->radius > 0.0) || !(o->radius <= 1024.0) || std::isnan(o->ref_resolution))) return VIL_ERR_INVALID_ARGUMENT;
    if (!all_finite(xyz, 3 * (size_t)n) || !all_finite(T16, 12) || (T_out16 && !all_finite(T_out16, 12))) return VIL_ERR_NON_FINITE;
    *n_ref = 0;
    if (c->n_map == 0) return VIL_OK;
    VILCHK(hipSetDevice(c->device));
    const int nm = c->n_map, nbm = nblk(nm), max_ref = c->cfg.max_ref_points;
    // the search grid: cell edge a power of two (exact cell indices), in radius mode not below the radius; rebuilt when the map has changed
    float want_h = c->grid_valid ? c->grid_h : 0.5f;
    if (!knn) { want_h = 1.f / 1024.f; while ((double)want_h < o->radius) want_h *= 2.f; }
    VILCHK(c->prof.mark(0, c->stream));
    const bool regrid = !c->grid_valid || want_h != c->grid_h;
    if (regrid) {
        c->grid_valid = false;
        VILCHK(vknn::grid_build(c->gb, nm, c->at<float>(c->o_map), 3, want_h, c->stream));
        c->grid_h = want_h; c->grid_valid = true;
    }
    VILCHK(c->prof.mark(1, c->stream));
    int* rec = c->at<int>(c->o_rec);
    const Seg* d_seg = c->at<Seg>(c->o_seg);
    memcpy(c->h_in, xyz, 12 * (size_t)n);
    set_seg(c->h_seg[0], T16, 0, 0);
    if (T_out16) set_seg(c->h_seg[1], T_out16, 0, 0);
    VILCHK(hipMemsetAsync(rec, 0, 16, c->stream));
    VILCHK(hipMemcpyAsync(c->d_mem + c->o_in, c->h_in, 12 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    VILCHK(hipMemcpyAsync(c->d_mem + c->o_seg, c->h_seg, 2 * sizeof(Seg), hipMemcpyHostToDevice, c->stream));
    const float* d_in = c->at<float>(c->o_in); const float* d_map = c->at<float>(c->o_map);
    int* d_mark = c->at<int>(c->o_mark); int* d_slot = c->at<int>(c->o_mslot); int* d_blk = c->at<int>(c->o_blk); int* d_off = c->at<int>(c->o_off);
    float* d_rxyz = c->at<float>(c->o_rxyz); int* d_ridx = c->at<int>(c->o_ridx);
    const int nqb = (n + VG_QPB - 1) / VG_QPB;
    const bool thin = !knn && o->ref_resolution > 0.f;
    Tab st = c->scratch();
    VILCHK(c->prof.mark(2, c->stream));
    if (knn) {
        int* d_kj = c->at<int>(c->o_knnj); int* d_kc = c->at<int>(c->o_knnc);
        hipLaunchKernelGGL(k_gmap_knn, dim3(nqb), dim3(64 * VG_QPB), 0, c->stream, n, d_in, d_seg, o->k, o->max_dist, o->max_dist * 1.001f + 1e-30f, nm, c->gb.G, c->gb.order, c->gb.cxyz, d_kj, d_kc);
        VILCHK(c->prof.mark(3, c->stream));
        hipLaunchKernelGGL(k_gmap_scan, dim3(1), dim3(VG_SCAN), 0, c->stream, n, d_kc, d_off, 0, rec);
        VILCHK(c->prof.mark(4, c->stream));
        hipLaunchKernelGGL(k_gmap_emit, dim3(nblk(n * o->k)), dim3(VG_BLK), 0, c->stream, n * o->k, d_map, d_mark, 0, false, st, d_slot, d_off, d_kj, d_kc, o->k, d_seg, T_out16 != nullptr, max_ref,
                           d_rxyz, d_ridx, rec);
        VILCHK(c->prof.mark(5, c->stream));
    } else {
        if (c->epoch == INT_MAX) { VILCHK(hipMemsetAsync(d_mark, 0, 4 * (size_t)c->cfg.max_map_points, c->stream)); c->epoch = 0; }
        const int epoch = ++c->epoch;
        const double pad = o->radius * (1.0 + 1e-5);
        hipLaunchKernelGGL(k_gmap_radius, dim3(nqb), dim3(64 * VG_QPB), 0, c->stream, n, d_in, d_seg, (float)(o->radius * o->radius), pad, c->gb.G, c->gb.order, c->gb.cxyz, epoch, d_mark);
        VILCHK(c->prof.mark(3, c->stream));
        if (thin) hipLaunchKernelGGL(k_gmap_thin, dim3(nbm), dim3(VG_BLK), 0, c->stream, nm, d_map, d_mark, epoch, c->vox(o->ref_resolution), st, d_slot, rec);
        VILCHK(c->prof.mark(4, c->stream));
        hipLaunchKernelGGL(k_gmap_pick, dim3(nbm), dim3(VG_BLK), 0, c->stream, nm, d_mark, epoch, thin, st, d_slot, d_blk, rec);
        VILCHK(c->prof.mark(5, c->stream));
        hipLaunchKernelGGL(k_gmap_scan, dim3(1), dim3(VG_SCAN), 0, c->stream, nbm, d_blk, d_off, 0, rec);
        VILCHK(c->prof.mark(6, c->stream));
        hipLaunchKernelGGL(k_gmap_emit, dim3(nbm), dim3(VG_BLK), 0, c->stream, nm, d_map, d_mark, epoch, thin, st, d_slot, d_off, (const int*)nullptr, (const int*)nullptr, 1, d_seg,
                           T_out16 != nullptr, max_ref, d_rxyz, d_ridx, rec);
        VILCHK(c->prof.mark(7, c->stream));
        if (thin) hipLaunchKernelGGL(k_gmap_unclaim, dim3(nbm), dim3(VG_BLK), 0, c->stream, nm, d_mark, epoch, st, d_slot);
        VILCHK(c->prof.mark(8, c->stream));
    }
    VILCHK(hipMemcpyAsync(c->h_rec, rec, 16, hipMemcpyDeviceToHost, c->stream));
    VILCHK(hipStreamSynchronize(c->stream));
    VILCHK(hipGetLastError());
    if (regrid) c->prof.span(K_GRID, 0, 1);
    if (knn) { c->prof.span(K_KNN, 2, 3); c->prof.span(K_SCAN, 3, 4); c->prof.span(K_EMIT, 4, 5); }
    else {
        c->prof.span(K_RADIUS, 2, 3);
        if (thin) { c->prof.span(K_THIN, 3, 4); c->prof.span(K_UNCLAIM, 7, 8); }
        c->prof.span(K_PICK, 4, 5); c->prof.span(K_SCAN, 5, 6); c->prof.span(K_EMIT, 6, 7);
    }
    if (c->h_rec[0]) return VIL_ERR_INVALID_ARGUMENT;       // a reference voxel index outside 2^20
    if (c->h_rec[2]) return VIL_ERR_CAPACITY;               // unreachable, as in submit_insert
    const int nr = c->h_rec[1];
    *n_ref = nr;
    if (nr > max_ref) return VIL_ERR_CAPACITY;
    if (nr == 0) return VIL_OK;
    VILCHK(hipMemcpyAsync(c->h_out, d_rxyz, 12 * (size_t)nr, hipMemcpyDeviceToHost, c->stream));
    if (ref_idx) VILCHK(hipMemcpyAsync(c->h_out + 12 * (size_t)max_ref, d_ridx, 4 * (size_t)nr, hipMemcpyDeviceToHost, c->stream));
    VILCHK(hipStreamSynchronize(c->stream));
    memcpy(ref_xyz, c->h_out, 12 * (size_t)nr);
    if (ref_idx) memcpy(ref_idx, c->h_out + 12 * (size_t)max_ref, 4 * (size_t)nr);
    return VIL_OK;
}

}  // extern "C"
