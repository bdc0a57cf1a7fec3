// vilcloud_dev.hpp -- the device pieces of filter A (include/vilcloud.h) that more than one launch structure runs: vilcloud.hip spreads ONE
// cloud over many workgroups (k_cloud_*), villmap.hip gives every cube of the local map ONE workgroup of its own (k_lmap_refilter).  The
// voxel and its table entry, the stable ranking of 64 points by ballots, the eviction flag and the sequential sum of a run are written
// here once; what differs between the two is only who owns which points and where the histograms live.
// csrc-internal, device code only.  The including file keeps the contract's arithmetic unfused (#pragma clang fp contract(off)) BEFORE
// it includes this header.
#pragma once
#include <hip/hip_runtime.h>

namespace vilcloud_dev {

__device__ __forceinline__ bool same_voxel(const int4 a, const int4 b) { return a.x == b.x && a.y == b.y && a.z == b.z && a.w == b.w; }
__device__ __forceinline__ bool fits_int(const float f) { return f >= -2147483648.0f && f < 2147483648.0f; }      // false for NaN

// steps 1-2 and the DEVIATION: (ix, iy, iz, bucket), bucket -1 for a dropped point
__device__ __forceinline__ int4 voxel_of(const float4 p, const float inv, const unsigned hmask) {
    const float fx = floorf(p.x * inv), fy = floorf(p.y * inv), fz = floorf(p.z * inv);
    if (!(isfinite(p.x) && isfinite(p.y) && isfinite(p.z) && fits_int(fx) && fits_int(fy) && fits_int(fz))) return make_int4(0, 0, 0, -1);
    const int ix = (int)fx, iy = (int)fy, iz = (int)fz;
    const unsigned h = ((unsigned)ix * 7171u + (unsigned)iy * 3079u + (unsigned)iz * 4231u) & hmask;
    return make_int4(ix, iy, iz, (int)h);
}

// One wave ranks the points i0 .. i0 + 64 * steps (those below n), 64 at a time in index order.  hist: the wave's own counters, one per
// bucket.  SCATTER = false: they end as the piece's histogram (the caller zeroed them); SCATTER = true: they start at the piece's offsets
// and every point's index goes to its place in `sorted`.  A lane finds the lanes of its wave with the same bucket with one ballot per
// bucket bit; its rank among them is a popcount.  Every wave of the workgroup takes the same number of steps, so the barriers are uniform;
// a wave only ever touches its own counters.
template <bool SCATTER>
__device__ __forceinline__ void rank_piece(const int i0, const int steps, const int n, const int4* vox, const int bits, int* sorted, int* hist) {
    const int lane = threadIdx.x & 63;
    for (int step = 0; step < steps; ++step) {
        const int i = i0 + step * 64 + lane;
        const int h = i < n ? vox[i].w : -1;
        const bool valid = h >= 0;
        unsigned long long same = __ballot(valid);
        for (int bit = 0; bit < bits; ++bit) {
            const bool one = (h >> bit) & 1;
            const unsigned long long bb = __ballot(one);
            same &= one ? bb : ~bb;
        }
        const int rank = __popcll(same & ((1ull << lane) - 1ull));
        const int old = valid ? hist[h] : 0;                                                       // h < H: the bucket was masked with H - 1
        __syncthreads();
        if (valid && rank == 0) hist[h] = old + __popcll(same);
        if (SCATTER && valid) sorted[old + rank] = i;                                              // old + rank < points that are not dropped <= n
        __syncthreads();
    }
}

// sorted place p >= 1 of nv: the start of a run that has a predecessor in its bucket is where step 3 evicts; flagged at its ORIGINAL index
__device__ __forceinline__ void flag_eviction(const int p, const int4* vox, const int* sorted, int* evict) {
    const int i = sorted[p];                                                                       // sorted holds indices < n of points that were not dropped
    const int4 v = vox[i], u = vox[sorted[p - 1]];
    if (u.w == v.w && !same_voxel(u, v)) evict[i] = 1;
}

// steps 3-5 for sorted place p < nv: nothing unless a run starts there; else the run's centroid, summed sequentially from 0.0f in index
// order, to its output position.  evpos: the exclusive sum of the eviction flags in original index order; brank[b]: the non-empty
// buckets before b.
__device__ __forceinline__ void emit_run(const int p, const int nv, const int n_evict, const float4* in, const int4* vox, const int* sorted, const int* evpos, const int* brank,
                                         float4* out) {
    const int i = sorted[p];
    const int4 v = vox[i];
    if (p > 0 && same_voxel(vox[sorted[p - 1]], v)) return;                                        // not a run start
    float sx = 0.0f, sy = 0.0f, sz = 0.0f, sw = 0.0f;
    int cnt = 0, q = p, j = i;
    int4 u = v;
    do {                                                                                           // step 4, in index order
        const float4 pt = in[j];
        sx = sx + pt.x; sy = sy + pt.y; sz = sz + pt.z; sw = sw + pt.w;
        ++cnt; ++q;
        if (q < nv) { j = sorted[q]; u = vox[j]; }
    } while (q < nv && same_voxel(u, v));
    const float c = (float)cnt;
    // a successor in the bucket: flushed when the successor's first point arrives, position = the evictions before that point; the bucket's
    // last run: flushed at the end.  evpos[j] < n_evict and n_evict + brank < runs <= n: inside `out`
    const int pos = (q < nv && u.w == v.w) ? evpos[j] : n_evict + brank[v.w];
    out[pos] = make_float4(sx / c, sy / c, sz / c, sw / c);
}

}  // namespace vilcloud_dev
