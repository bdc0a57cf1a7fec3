// vil_voxmap.hpp -- VGICP's target voxel map: the set of arrays a map lives in (VoxSet) and the device builder (build_target_dev).
// Part of vilvgicp.hip's translation unit, which includes it between its own kernels, after VG_THREADS, pack_key and hash_key.
#pragma once
#include "../../include/vilvgicp.h"
#include "vil_host.hpp"

namespace {

// One voxel map: the open-addressing table (tcap slots in use: packed 63-bit key -> voxel number) and the voxel records (SoA, voxel
// order; wsq = sqrt(num)).  A context holds two, the live target and the one the builders fill aside.
struct VoxSet {
    vilhost::Grown<long long> keys; vilhost::Grown<int> slot, num; vilhost::Grown<double> mean, cov, wsq;
    int tcap = 0, nvox = 0; double res = 1.0;
};

// ---- the target voxel map on the device (docs/voxelmap.md): GaussianVoxelMap::create_voxelmap's sequential sums, reproduced bit for bit.
// Membership by an open-addressing table (64-bit compare-and-swap, as vknn::grid_slot); a voxel's number is the count of "first point of
// its voxel" flags below its first point (atomicMin per slot + a prefix sum over the points); every voxel's members are put into ascending
// index order by ranking them inside the voxel's run, and one lane per (voxel, component) then adds the run in that order from 0.0 -- the
// host loop's additions, one by one.  Integer atomics only: which slot a key lands in and where a run lies depend on timing, no result does.
struct VoxBuild {
    long long* keys; int* slot_vox; int mask;             // the table being built (the set aside, not the live target)
    int* cnt; int* cur; int* start; unsigned* first;      // per table slot: members, fill cursor, start of the run, smallest member
    int* pslot; int* member; int* sorted; int* vstart;    // per point: its slot, the runs as filled, the runs in index order; per voxel: start of its run
    int* bsum; int* boff;                                 // per 256 points: first-point flags in the block, and in all blocks before it
    int* ctr;                                             // [0] run cursor, [1] voxels, [2] non-finite flag
    int* num; double* mean; double* cov; double* wsq;     // the voxel records (SoA, voxel order)
};

__device__ __forceinline__ long long vox_key_exact(float x, float y, float z, double res) {
#pragma clang fp contract(off)
    const double px = (double)x, py = (double)y, pz = (double)z;          // IEEE divide, subtract, floor: the host's expression, operation by operation
    return pack_key((int)floor(px / res - 0.5), (int)floor(py / res - 0.5), (int)floor(pz / res - 0.5));
}

// every slot of the table in use empty, the counters zero: nothing of an earlier (larger) build is read again
__global__ __launch_bounds__(VG_THREADS) void k_vox_clear(int tcap, VoxBuild B) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < 4) B.ctr[e] = 0;
    if (e >= tcap) return;
    B.keys[e] = -1LL; B.slot_vox[e] = -1; B.cnt[e] = 0; B.cur[e] = 0; B.first[e] = 0xFFFFFFFFu;
}
__global__ __launch_bounds__(VG_THREADS) void k_vox_insert(int n, const float* __restrict__ xyz, double res, VoxBuild B) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float x = xyz[3 * (size_t)i], y = xyz[3 * (size_t)i + 1], z = xyz[3 * (size_t)i + 2];
    if (!(isfinite(x) && isfinite(y) && isfinite(z))) { B.pslot[i] = -1; atomicOr(B.ctr + 2, 1); return; }
    const long long key = vox_key_exact(x, y, z, res);
    int s = -1;
    for (unsigned h = hash_key(key) & B.mask;; h = (h + 1) & B.mask) {      // at most n keys in >= 2 n slots: never full
        long long k = B.keys[h];
        if (k < 0) k = (long long)atomicCAS((unsigned long long*)(B.keys + h), (unsigned long long)-1LL, (unsigned long long)key);      // a stale -1 is settled here
        if (k < 0 || k == key) { s = (int)h; break; }
    }
    B.pslot[i] = s;
    atomicAdd(B.cnt + s, 1);
    atomicMin(B.first + s, (unsigned)i);
}
// every occupied slot claims a contiguous run (where it lies is irrelevant, as in vknn::k_grid_offsets)
__global__ __launch_bounds__(VG_THREADS) void k_vox_offsets(int tcap, VoxBuild B) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= tcap) return;
    const int c = B.cnt[e];
    if (c) B.start[e] = atomicAdd(B.ctr, c);
}
// members into their runs in arrival order; the block's number of first points for the numbering
__global__ __launch_bounds__(VG_THREADS) void k_vox_fill(int n, VoxBuild B) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int s = i < n ? B.pslot[i] : -1;
    if (s >= 0) B.member[B.start[s] + atomicAdd(B.cur + s, 1)] = i;
    const int firsts = __syncthreads_count(s >= 0 && B.first[s] == (unsigned)i);
    if (threadIdx.x == 0) B.bsum[blockIdx.x] = firsts;
}
// exclusive prefix sum of the block counts by one workgroup, 256 at a time with a carry; the total is the number of voxels
__global__ __launch_bounds__(VG_THREADS) void k_vox_scan(int nb, VoxBuild B) {
    __shared__ int wtot[VG_THREADS / 64];
    __shared__ int carry_sh;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (t == 0) carry_sh = 0;
    __syncthreads();
    for (int base = 0; base < nb; base += VG_THREADS) {
        const int x = base + t < nb ? B.bsum[base + t] : 0;
        int incl = x;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int v = __shfl_up(incl, o, 64); incl += lane >= o ? v : 0; }
        if (lane == 63) wtot[wave] = incl;
        __syncthreads();
        int woff = 0;
        for (int w = 0; w < wave; ++w) woff += wtot[w];
        const int carry = carry_sh;
        if (base + t < nb) B.boff[base + t] = carry + woff + incl - x;
        __syncthreads();
        if (t == VG_THREADS - 1) carry_sh = carry + woff + incl;
        __syncthreads();
    }
    if (t == 0) B.ctr[1] = carry_sh;
}
// numbering: a voxel's number is the count of first points before its own; ranking: a member's place in its run is the count of smaller members
__global__ __launch_bounds__(VG_THREADS) void k_vox_rank(int n, VoxBuild B) {
    __shared__ int wtot[VG_THREADS / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int i = blockIdx.x * blockDim.x + t;
    const int s = i < n ? B.pslot[i] : -1;
    const bool is_first = s >= 0 && B.first[s] == (unsigned)i;
    const unsigned long long bal = __ballot(is_first);
    if (lane == 0) wtot[wave] = __popcll(bal);
    __syncthreads();
    if (s < 0) return;
    const int b = B.start[s], c = B.cnt[s];
    if (is_first) {
        int v = B.boff[blockIdx.x] + __popcll(bal & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; ++w) v += wtot[w];
        B.slot_vox[s] = v; B.vstart[v] = b; B.num[v] = c; B.wsq[v] = sqrt((double)c);
    }
    int r = 0;
    for (int q = 0; q < c; ++q) r += B.member[b + q] < i ? 1 : 0;
    B.sorted[b + r] = i;
}
// one lane per (voxel, component): 3 of the mean, 9 of the covariance; the run in ascending point index, starting from 0.0
__global__ __launch_bounds__(VG_THREADS) void k_vox_sum(const float* __restrict__ xyz, const double* __restrict__ cov9, VoxBuild B) {
#pragma clang fp contract(off)
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int v = (int)(tid / 12), q = (int)(tid - 12 * (long long)v);
    if (v >= B.ctr[1]) return;
    const int b = B.vstart[v], c = B.num[v];
    double acc = 0.0;
    int u = 0;
    for (; u + 4 <= c; u += 4) {                          // the loads of four members go out together, the additions stay in order
        const int i0 = B.sorted[b + u], i1 = B.sorted[b + u + 1], i2 = B.sorted[b + u + 2], i3 = B.sorted[b + u + 3];
        const double a0 = q < 3 ? (double)xyz[3 * (size_t)i0 + q] : cov9[9 * (size_t)i0 + q - 3], a1 = q < 3 ? (double)xyz[3 * (size_t)i1 + q] : cov9[9 * (size_t)i1 + q - 3];
        const double a2 = q < 3 ? (double)xyz[3 * (size_t)i2 + q] : cov9[9 * (size_t)i2 + q - 3], a3 = q < 3 ? (double)xyz[3 * (size_t)i3 + q] : cov9[9 * (size_t)i3 + q - 3];
        acc += a0; acc += a1; acc += a2; acc += a3;
    }
    for (; u < c; ++u) { const int i = B.sorted[b + u]; acc += q < 3 ? (double)xyz[3 * (size_t)i + q] : cov9[9 * (size_t)i + q - 3]; }
    const double m = acc / (double)c;                     // finalize(): the IEEE divide
    if (q < 3) B.mean[3 * (size_t)v + q] = m; else B.cov[9 * (size_t)v + q - 3] = m;
}

// The map of n device-resident points and covariances, built into `a` (the set aside: the caller installs it when this returns VIL_OK and
// keeps its target on VIL_ERR_NON_FINITE or a HIP error).  Seven launches, then ONE host wait for the voxel count and the non-finite
// flag in h_build (pinned, two ints).  ws: the build's work space, grown on demand.
int build_target_dev(VoxSet& a, vilhost::Grown<char>& ws, vilhost::Profiler<VGICP_BUILD_KERNELS, VGICP_BUILD_KERNELS + 1>& prof, int* h_build, hipStream_t s,
                     int n, const float* d_xyz, const double* d_cov9, double resolution) {
    if (n > (1 << 28)) return VIL_ERR_CAPACITY;          // (2 n table slots and 12 n lanes stay below 2^31 with room to spare)
    int tcap = 64; while (tcap < 2 * n) tcap <<= 1;     // sized from n: the number of voxels is not known on the host
    const size_t v = (size_t)n + (size_t)n / 2;          // head room: the next scans are about this size
    VILCHK(a.keys.reserve(tcap, tcap)); VILCHK(a.slot.reserve(tcap, tcap)); VILCHK(a.num.reserve(n, v));
    VILCHK(a.mean.reserve(3 * (size_t)n, 3 * v)); VILCHK(a.cov.reserve(9 * (size_t)n, 9 * v)); VILCHK(a.wsq.reserve(n, v));
    const int nb = (n + VG_THREADS - 1) / VG_THREADS;
    vilhost::Arena ar;
    const size_t o_cnt = ar.take(4 * (size_t)tcap), o_cur = ar.take(4 * (size_t)tcap), o_start = ar.take(4 * (size_t)tcap), o_first = ar.take(4 * (size_t)tcap);
    const size_t o_pslot = ar.take(4 * (size_t)n), o_member = ar.take(4 * (size_t)n), o_sorted = ar.take(4 * (size_t)n), o_vstart = ar.take(4 * (size_t)n);
    const size_t o_bsum = ar.take(4 * (size_t)nb), o_boff = ar.take(4 * (size_t)nb), o_ctr = ar.take(16);
    VILCHK(ws.reserve(ar.bytes, ar.bytes + ar.bytes / 2));
    char* w = ws.p;
    VoxBuild B{a.keys.p, a.slot.p, tcap - 1, (int*)(w + o_cnt), (int*)(w + o_cur), (int*)(w + o_start), (unsigned*)(w + o_first),
               (int*)(w + o_pslot), (int*)(w + o_member), (int*)(w + o_sorted), (int*)(w + o_vstart), (int*)(w + o_bsum), (int*)(w + o_boff), (int*)(w + o_ctr),
               a.num.p, a.mean.p, a.cov.p, a.wsq.p};
    const dim3 T(VG_THREADS), Gt((tcap + VG_THREADS - 1) / VG_THREADS), Gn(nb), Gs((unsigned)((12 * (size_t)n + VG_THREADS - 1) / VG_THREADS));
    VILCHK(prof.mark(0, s)); hipLaunchKernelGGL(k_vox_clear, Gt, T, 0, s, tcap, B);
    VILCHK(prof.mark(1, s)); hipLaunchKernelGGL(k_vox_insert, Gn, T, 0, s, n, d_xyz, resolution, B);
    VILCHK(prof.mark(2, s)); hipLaunchKernelGGL(k_vox_offsets, Gt, T, 0, s, tcap, B);
    VILCHK(prof.mark(3, s)); hipLaunchKernelGGL(k_vox_fill, Gn, T, 0, s, n, B);
    VILCHK(prof.mark(4, s)); hipLaunchKernelGGL(k_vox_scan, dim3(1), T, 0, s, nb, B);
    VILCHK(prof.mark(5, s)); hipLaunchKernelGGL(k_vox_rank, Gn, T, 0, s, n, B);
    VILCHK(prof.mark(6, s)); hipLaunchKernelGGL(k_vox_sum, Gs, T, 0, s, d_xyz, d_cov9, B);
    VILCHK(prof.mark(7, s));
    VILCHK(hipMemcpyAsync(h_build, B.ctr + 1, 8, hipMemcpyDeviceToHost, s));
    VILCHK(hipStreamSynchronize(s));
    VILCHK(hipGetLastError());
    for (int k = 0; k < VGICP_BUILD_KERNELS; ++k) prof.span(k, k, k + 1);
    if (h_build[1]) return VIL_ERR_NON_FINITE;
    a.tcap = tcap; a.nvox = h_build[0]; a.res = resolution;
    return VIL_OK;
}

}  // namespace
