// vilcloud.hip -- the feature tracker's accumulated depth cloud, resident on gfx950, and an exact ApproximateVoxelGrid, behind
// include/vilcloud.h (feature_tracker_/src/feature_tracker_node.cpp: lidar_callback :252-337; the steps are numbered as in the header).
//
// FILTER A is order-dependent but not sequential: what a table entry does depends only on the points that hash into it.  So
//   k_cloud_keys     a thread per point: the voxel, the table entry ("bucket") and the drop flag (steps 1-2 and the DEVIATION).
//   k_cloud_count    a STABLE one-pass counting sort by bucket.  A workgroup owns VC_WG_PTS consecutive points, each of its four waves
//   k_cloud_scan     VC_WAVE_PTS consecutive ones of them (a "segment"), taken 64 at a time in index order.  A lane finds the lanes of its
//   k_cloud_scatter  wave with the same bucket with one ballot per bucket bit; its rank among them is a popcount, the bucket's count so far
//                    is the wave's own histogram in LDS.  k_cloud_count leaves the histograms in a (bucket-major, segment-minor) table,
//                    k_cloud_scan turns the table into offsets (one workgroup, an exclusive sum in place), k_cloud_scatter repeats the
//                    ranking from those offsets and writes the point's index to its place.  Within a bucket the points keep index order.
//   k_cloud_runs     a thread per sorted point: it starts a RUN when its voxel differs from its predecessor's or it is the first of its
//                    bucket.  A run is what the entry holds between two flushes.  A run start that is not the first of its bucket is
//                    the point at which step 3 evicts the run before it: it is flagged at its ORIGINAL index.
//   k_cloud_scan     the exclusive sum of the flags in original index order: the output position of every eviction (step 3's "next output
//                    position"), and their number.
//   k_cloud_buckets  the rank of every bucket among the non-empty ones: the final flush (step 5) follows the evictions in bucket order.
//   k_cloud_emit     a thread per run start walks its run in order and adds sequentially from 0.0f -- the sequential float sum IS the
//                    contract, so a long run is one thread's loop (DESIGN.md section 8.11 says what that costs) -- divides, and writes the
//                    centroid where its successor's flag sum says, or, for the last run of a bucket, behind the evictions.
// No atomics anywhere: nothing depends on the order in which workgroups run.
//
// ACCUMULATION: A(leaf_scan) on the upload, then
//   k_cloud_view     a thread per centroid: the keep flag of step 2 (k_cloud_scan sums the flags),
//   k_cloud_place    the ordered compaction fused with step 3's transform, into the scan's slot of the queue,
//   k_cloud_fuse     step 5: a gather over the live slots by the prefix of their counts, oldest first,
// and A(leaf_cloud) on the fused cloud.  The queue is a ring of max_scans slots; which slots are live is decided on the host from the
// stamps (step 4), every point count is read by the kernels from a header on the device, grids are sized from upper bounds the host
// knows (a scan in the queue has at most as many points as were handed over).
// The float arithmetic of the contract is kept unfused and in source order (hipcc would contract a * b + c):
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/vilcloud.h"
#include "vil_host.hpp"
#include "vilcloud_dev.hpp"
#include "vilcloud_stage.hpp"
#include "vildepth_stage.hpp"

#define VC_BLK 256
#define VC_WAVES (VC_BLK / 64)
#define VC_WAVE_PTS 1024                     // a segment: the points one wave ranks, 16 steps of 64
#define VC_WG_PTS (VC_WAVES * VC_WAVE_PTS)
#define VC_SCAN 1024                         // threads of k_cloud_scan and k_cloud_buckets
#define VC_MAX_POINTS (1 << 27)

namespace {

enum { K_KEYS = 0, K_COUNT, K_SCAN, K_SCATTER, K_RUNS, K_BUCKETS, K_EMIT, K_VIEW, K_PLACE, K_FUSE };
static_assert(K_FUSE + 1 == VCLOUD_NUM_KERNELS, "one profile entry per kernel");
// the device header (ints): the point counts of one push, of one vcloud_filter, and the three counts filter A keeps for itself
enum { H_RAW = 0, H_DS, H_VIEW, H_FUSED, H_CLOUD, H_FIN, H_FOUT, H_VALID, H_EVICT, H_NONEMPTY, H_INTS = 16 };

// the voxel, the ranking by ballots, the eviction flag and the run's sum are shared with villmap.hip's one-workgroup-per-cube filter
using namespace vilcloud_dev;

// steps 1-2: vox[i] = (ix, iy, iz, bucket), bucket -1 for a dropped point and for i >= n; the eviction flags are cleared
__global__ __launch_bounds__(VC_BLK) void k_cloud_keys(const int* __restrict__ d_n, int n_upper, const float4* __restrict__ in, float inv, unsigned hmask,
                                                       int4* __restrict__ vox, int* __restrict__ evict) {
    const int i = blockIdx.x * VC_BLK + threadIdx.x;
    if (i >= n_upper) return;
    evict[i] = 0;
    vox[i] = i < *d_n ? voxel_of(in[i], inv, hmask) : make_int4(0, 0, 0, -1);
}

// The ranking both sort passes share (rank_piece of vilcloud_dev.hpp) for a wave's segment.  hist: the wave's H counters.  SCATTER = false:
// they start at 0 and end as the segment's histogram; SCATTER = true: they start at the segment's offsets.
template <bool SCATTER>
__device__ __forceinline__ void rank_segment(const int n, const int4* __restrict__ vox, const int H, const int bits, const int nseg, int* __restrict__ table,
                                             int* __restrict__ sorted, int* hist) {
    const int lane = threadIdx.x & 63, seg = blockIdx.x * VC_WAVES + (threadIdx.x >> 6);
    for (int b = lane; b < H; b += 64) hist[b] = SCATTER ? table[(size_t)b * nseg + seg] : 0;
    __syncthreads();
    rank_piece<SCATTER>(seg * VC_WAVE_PTS, VC_WAVE_PTS / 64, n, vox, bits, sorted, hist);
    if (!SCATTER) for (int b = lane; b < H; b += 64) table[(size_t)b * nseg + seg] = hist[b];
}

__global__ __launch_bounds__(VC_BLK) void k_cloud_count(const int* __restrict__ d_n, int n_upper, const int4* __restrict__ vox, int H, int bits, int nseg, int* __restrict__ table) {
    __shared__ int s_hist[VC_WAVES][VCLOUD_MAX_HIST];
    rank_segment<false>(min(*d_n, n_upper), vox, H, bits, nseg, table, nullptr, s_hist[threadIdx.x >> 6]);
}

__global__ __launch_bounds__(VC_BLK) void k_cloud_scatter(const int* __restrict__ d_n, int n_upper, const int4* __restrict__ vox, int H, int bits, int nseg, int* __restrict__ table,
                                                          int* __restrict__ sorted) {
    __shared__ int s_hist[VC_WAVES][VCLOUD_MAX_HIST];
    rank_segment<true>(min(*d_n, n_upper), vox, H, bits, nseg, table, sorted, s_hist[threadIdx.x >> 6]);
}

// the exclusive sum of every thread's own partial sum over the workgroup, and the sum of all of them
__device__ __forceinline__ int block_exclusive(const int s, int* s_w, int& all) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = s;
    for (int o = 1; o < 64; o <<= 1) { const int v = __shfl_up(inc, o); if (lane >= o) inc += v; }
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    int before = 0; all = 0;
    for (int w = 0; w < VC_SCAN / 64; ++w) { const int c = s_w[w]; before += w < wave ? c : 0; all += c; }
    return before + inc - s;
}

// four consecutive ints at a + j (j a multiple of 4, a 16-byte aligned), as one 16-byte access where they all lie below len
typedef int vint4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ vint4 load4(const int* a, const int j, const int len) {
    if (j + 3 < len) return *(const vint4*)(a + j);
    vint4 v = {0, 0, 0, 0};
    if (j < len) v.x = a[j];
    if (j + 1 < len) v.y = a[j + 1];
    if (j + 2 < len) v.z = a[j + 2];
    return v;
}
__device__ __forceinline__ void store4(int* a, const int j, const int len, const vint4 v) {
    if (j + 3 < len) { *(vint4*)(a + j) = v; return; }
    if (j < len) a[j] = v.x;
    if (j + 1 < len) a[j + 1] = v.y;
    if (j + 2 < len) a[j + 2] = v.z;
}

// a[0 .. len) becomes its exclusive prefix sum, *total the sum.  ONE workgroup; a wave owns a contiguous piece of whole 256-element
// tiles, which it reads and writes as coalesced 1 kB accesses (a lane's 16 bytes next to its neighbour's): a pass that adds the piece
// up, the pieces' sums through LDS, a pass that scans tile by tile with a carry.
__global__ __launch_bounds__(VC_SCAN) void k_cloud_scan(int* __restrict__ a, int len, int* __restrict__ total) {
    __shared__ int s_w[VC_SCAN / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tiles = (len + 255) / 256, per = (tiles + VC_SCAN / 64 - 1) / (VC_SCAN / 64);
    const int t0 = min(wave * per, tiles), t1 = min(t0 + per, tiles);
    int s = 0;
#pragma unroll 4
    for (int t = t0; t < t1; ++t) { const vint4 v = load4(a, t * 256 + lane * 4, len); s += (v.x + v.y) + (v.z + v.w); }
    for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) s_w[wave] = s;
    __syncthreads();
    int carry = 0, all = 0;
    for (int w = 0; w < VC_SCAN / 64; ++w) { const int c = s_w[w]; carry += w < wave ? c : 0; all += c; }
    for (int t = t0; t < t1; ++t) {
        const int j = t * 256 + lane * 4;
        const vint4 v = load4(a, j, len);
        const int mine = (v.x + v.y) + (v.z + v.w);
        int inc = mine;
        for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(inc, o); if (lane >= o) inc += u; }
        vint4 out;
        out.x = carry + inc - mine; out.y = out.x + v.x; out.z = out.y + v.y; out.w = out.z + v.z;
        store4(a, j, len, out);
        carry += __shfl(inc, 63);
    }
    if (threadIdx.x == 0) *total = all;
}

// run starts; the start of a run that has a predecessor in its bucket is where step 3 evicts
__global__ __launch_bounds__(VC_BLK) void k_cloud_runs(const int* __restrict__ hdr, int n_upper, const int4* __restrict__ vox, const int* __restrict__ sorted, int* __restrict__ evict) {
    const int p = blockIdx.x * VC_BLK + threadIdx.x;
    if (p == 0 || p >= min(hdr[H_VALID], n_upper)) return;
    flag_eviction(p, vox, sorted, evict);
}

// brank[b]: the non-empty buckets before b.  The bucket's first place is its entry of segment 0 in the offset table.
__global__ __launch_bounds__(VC_SCAN) void k_cloud_buckets(int* __restrict__ hdr, int H, int nseg, const int* __restrict__ table, int* __restrict__ brank) {
    __shared__ int s_w[VC_SCAN / 64];
    static_assert(VCLOUD_MAX_HIST == 2 * VC_SCAN, "two buckets per thread");
    const int b0 = 2 * threadIdx.x, nv = hdr[H_VALID];
    int f[2];
    for (int k = 0; k < 2; ++k) {
        const int b = b0 + k;
        f[k] = b < H ? ((b + 1 < H ? table[(size_t)(b + 1) * nseg] : nv) > table[(size_t)b * nseg]) : 0;
    }
    int all;
    const int ex = block_exclusive(f[0] + f[1], s_w, all);
    if (b0 < H) brank[b0] = ex;
    if (b0 + 1 < H) brank[b0 + 1] = ex + f[0];
    if (threadIdx.x == 0) hdr[H_NONEMPTY] = all;
}

// steps 3-5: the centroid of every run, to its output position
__global__ __launch_bounds__(VC_BLK) void k_cloud_emit(const int* hdr, int n_upper, const float4* __restrict__ in, const int4* __restrict__ vox, const int* __restrict__ sorted,
                                                       const int* __restrict__ evpos, const int* __restrict__ brank, float4* __restrict__ out, int* d_n_out) {
    const int p = blockIdx.x * VC_BLK + threadIdx.x;
    const int nv = min(hdr[H_VALID], n_upper), n_evict = hdr[H_EVICT];
    if (p == 0) *d_n_out = n_evict + hdr[H_NONEMPTY];
    if (p >= nv) return;
    emit_run(p, nv, n_evict, in, vox, sorted, evpos, brank, out);
}

// step 2 of the accumulation
__device__ __forceinline__ bool in_view(const float4 p, const float max_coord, const float max_ratio) {
    if (p.x > max_coord || p.y > max_coord || p.z > max_coord) return false;
    return p.x >= 0.0f && fabsf(p.y / p.x) <= max_ratio && fabsf(p.z / p.x) <= max_ratio;
}

__global__ __launch_bounds__(VC_BLK) void k_cloud_view(const int* __restrict__ d_n, int n_upper, const float4* __restrict__ ds, float max_coord, float max_ratio, int* __restrict__ flag) {
    const int k = blockIdx.x * VC_BLK + threadIdx.x;
    if (k >= n_upper) return;
    flag[k] = (k < *d_n && in_view(ds[k], max_coord, max_ratio)) ? 1 : 0;
}

// steps 2-3: the kept centroids, in order, transformed, into the scan's slot; the slot's count
__global__ __launch_bounds__(VC_BLK) void k_cloud_place(const int* __restrict__ hdr, int n_upper, const float4* __restrict__ ds, const int* __restrict__ pos, const float* __restrict__ M,
                                                        float max_coord, float max_ratio, float4* __restrict__ slot, int* __restrict__ slot_count) {
    const int k = blockIdx.x * VC_BLK + threadIdx.x;
    if (k == 0) *slot_count = hdr[H_VIEW];
    if (k >= min(hdr[H_DS], n_upper)) return;
    const float4 p = ds[k];
    if (!in_view(p, max_coord, max_ratio)) return;
    const float x = ((M[0] * p.x + M[1] * p.y) + M[2] * p.z) + M[3];
    const float y = ((M[4] * p.x + M[5] * p.y) + M[6] * p.z) + M[7];
    const float z = ((M[8] * p.x + M[9] * p.y) + M[10] * p.z) + M[11];
    slot[pos[k]] = make_float4(x, y, z, p.w);                                                       // pos[k] < kept centroids <= n_upper <= max_scan_points
}

// step 5: the live slots, `head` first, concatenated
__global__ __launch_bounds__(VC_BLK) void k_cloud_fuse(int* __restrict__ hdr, int n_upper, int head, int n_live, int max_scans, int max_scan_points, const int* __restrict__ slot_count,
                                                       const float4* __restrict__ slots, float4* __restrict__ fused) {
    __shared__ int s_pre[VCLOUD_MAX_SCANS + 1];
    if (threadIdx.x == 0) {
        int acc = 0;
        for (int s = 0; s < n_live; ++s) { s_pre[s] = acc; acc += min(slot_count[(head + s) % max_scans], max_scan_points); }
        s_pre[n_live] = acc;
    }
    __syncthreads();
    const int total = min(s_pre[n_live], n_upper);
    const int g = blockIdx.x * VC_BLK + threadIdx.x;
    if (g == 0) hdr[H_FUSED] = total;
    if (g >= total) return;
    int lo = 0, hi = n_live - 1;                                                                   // the last s with s_pre[s] <= g
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (s_pre[mid] <= g) lo = mid; else hi = mid - 1; }
    fused[g] = slots[(size_t)((head + lo) % max_scans) * max_scan_points + (g - s_pre[lo])];         // g - s_pre[lo] < that slot's count
}

bool finite_positive(const float v) { return std::isfinite(v) && v > 0.0f; }
int log2_of_hist(const int h) {                                                                    // -1 when h is not an accepted table size
    if (h < 1 || h > VCLOUD_MAX_HIST || (h & (h - 1))) return -1;
    int bits = 0;
    while ((1 << bits) < h) ++bits;
    return bits;
}
int segments_of(const int n_upper) { return VC_WAVES * ((n_upper + VC_WG_PTS - 1) / VC_WG_PTS); }

}  // namespace

struct vcloud_ctx : vilhost::Device {        // d_mem: header | matrix, raw scan | down-sampled scan | slot counts | queue | fused | cloud | filter in | filter out | work
    int msp = 0, ms = 0;                                    // max_scan_points, max_scans
    size_t ntot = 0;
    char* h_io = nullptr; int* h_hdr = nullptr;             // pinned: 64 bytes of matrix + points in either direction; the header
    size_t o_hdr = 0, o_up = 0, o_ds = 0, o_slotcnt = 0, o_slots = 0, o_fused = 0, o_cloud = 0, o_fin = 0, o_fout = 0, o_vox = 0, o_sorted = 0, o_evict = 0, o_table = 0, o_brank = 0;
    // the queue (step 4): ring of slots, `head` the oldest
    int head = 0, n_live = 0, n_cloud = 0;
    double stamps[VCLOUD_MAX_SCANS] = {};
    int counts[VCLOUD_MAX_SCANS] = {};                      // points per slot, as the summaries reported them
    int last_slot = -1, last_ds = 0, last_view = 0, last_fused = 0;    // what vcloud_debug_read reads
    vilhost::EventLog<VCLOUD_NUM_KERNELS> prof;

    template <class T> T* at(size_t o) { return (T*)(d_mem + o); }
};

namespace {

// Filter A, enqueue only: n = min(*d_n, n_upper) points of `in`, the centroids to `out` (room for n_upper), their number to *d_n_out
int enqueue_filter(vcloud_ctx* c, const float4* in, const int* d_n, const int n_upper_, const float leaf, const int H, float4* out, int* d_n_out) {
    const int n_upper = n_upper_ > 0 ? n_upper_ : 1, nseg = segments_of(n_upper), bits = log2_of_hist(H), blocks = (n_upper + VC_BLK - 1) / VC_BLK;
    const float inv = 1.0f / leaf;
    int* hdr = c->at<int>(c->o_hdr); int4* vox = c->at<int4>(c->o_vox); int* sorted = c->at<int>(c->o_sorted); int* evict = c->at<int>(c->o_evict);
    int* table = c->at<int>(c->o_table); int* brank = c->at<int>(c->o_brank);
    hipStream_t q = c->stream;
    VILCHK(c->prof.mark(K_KEYS, 1, q));
    hipLaunchKernelGGL(k_cloud_keys, dim3(blocks), dim3(VC_BLK), 0, q, d_n, n_upper, in, inv, (unsigned)(H - 1), vox, evict);
    VILCHK(c->prof.mark(K_COUNT, 1, q));
    hipLaunchKernelGGL(k_cloud_count, dim3(nseg / VC_WAVES), dim3(VC_BLK), 0, q, d_n, n_upper, vox, H, bits, nseg, table);
    VILCHK(c->prof.mark(K_SCAN, 1, q));
    hipLaunchKernelGGL(k_cloud_scan, dim3(1), dim3(VC_SCAN), 0, q, table, H * nseg, hdr + H_VALID);
    VILCHK(c->prof.mark(K_SCATTER, 1, q));
    hipLaunchKernelGGL(k_cloud_scatter, dim3(nseg / VC_WAVES), dim3(VC_BLK), 0, q, d_n, n_upper, vox, H, bits, nseg, table, sorted);
    VILCHK(c->prof.mark(K_RUNS, 1, q));
    hipLaunchKernelGGL(k_cloud_runs, dim3(blocks), dim3(VC_BLK), 0, q, hdr, n_upper, vox, sorted, evict);
    VILCHK(c->prof.mark(K_SCAN, 1, q));
    hipLaunchKernelGGL(k_cloud_scan, dim3(1), dim3(VC_SCAN), 0, q, evict, n_upper, hdr + H_EVICT);
    VILCHK(c->prof.mark(K_BUCKETS, 1, q));
    hipLaunchKernelGGL(k_cloud_buckets, dim3(1), dim3(VC_SCAN), 0, q, hdr, H, nseg, table, brank);
    VILCHK(c->prof.mark(K_EMIT, 1, q));
    hipLaunchKernelGGL(k_cloud_emit, dim3(blocks), dim3(VC_BLK), 0, q, hdr, n_upper, in, vox, sorted, evict, brank, out, d_n_out);
    return VIL_OK;
}

int read_points(vcloud_ctx* c, const size_t offset, const int n_have, float* out, const int32_t capacity, int32_t* n) {
    if (!n) return VIL_ERR_INVALID_ARGUMENT;
    *n = n_have;
    if (capacity < n_have || (n_have && !out)) return VIL_ERR_INVALID_ARGUMENT;
    if (n_have) {
        VILCHK(hipSetDevice(c->device));
        VILCHK(hipMemcpyAsync(out, c->d_mem + offset, 16 * (size_t)n_have, hipMemcpyDeviceToHost, c->stream));
        VILCHK(hipStreamSynchronize(c->stream));
    }
    return VIL_OK;
}

}  // namespace

bool vilcloud_stage::accepts(float leaf, int32_t hist_size) { return finite_positive(leaf) && log2_of_hist(hist_size) >= 0; }

int vilcloud_stage::filter_resident(vcloud_ctx* c, const float4* in, const int* d_n, int n_upper, float leaf, int32_t hist_size, float4* out, int* d_n_out, hipEvent_t ready,
                                    vilhost::Fence& done) {
    if (!c || !in || !d_n || !out || !d_n_out || !ready || n_upper < 0 || (size_t)n_upper > c->ntot || !accepts(leaf, hist_size)) return VIL_ERR_INVALID_ARGUMENT;
    VILCHK(hipSetDevice(c->device));
    VILCHK(hipStreamWaitEvent(c->stream, ready, 0));
    const int st = enqueue_filter(c, in, d_n, n_upper, leaf, hist_size, out, d_n_out);
    if (st != VIL_OK) return st;
    VILCHK(done.record(c->stream));
    return VIL_OK;
}

extern "C" {

void vcloud_default_options(vcloud_options* o) {
    if (!o) return;
    o->leaf_scan = 0.2f; o->leaf_cloud = 0.1f; o->hist_size = 512; o->max_coord = 25.0f; o->max_ratio = 10.0f; o->reserved = 0; o->window_s = 5.0;
}

int vcloud_create(int32_t device, int32_t max_scan_points, int32_t max_scans, vcloud_ctx** out) {
    if (!out || max_scan_points < 1 || max_scans < 1 || max_scans > VCLOUD_MAX_SCANS || (int64_t)max_scan_points * max_scans > VC_MAX_POINTS) return VIL_ERR_INVALID_ARGUMENT;
    vcloud_ctx* c = new vcloud_ctx();
    c->msp = max_scan_points; c->ms = max_scans;
    const size_t N = (size_t)max_scan_points, T = N * (size_t)max_scans;
    c->ntot = T;
    vilhost::Arena a;
    c->o_hdr = a.take(4 * H_INTS);
    c->o_up = a.take(64 + 16 * N);                          // the matrix and the raw scan go up as one copy
    c->o_ds = a.take(16 * N);
    c->o_slotcnt = a.take(4 * (size_t)max_scans);
    c->o_slots = a.take(16 * T);
    c->o_fused = a.take(16 * T);
    c->o_cloud = a.take(16 * T);
    c->o_fin = a.take(16 * T);
    c->o_fout = a.take(16 * T);
    c->o_vox = a.take(16 * T);
    c->o_sorted = a.take(4 * T);
    c->o_evict = a.take(4 * T + 16);
    c->o_table = a.take(4 * (size_t)VCLOUD_MAX_HIST * (size_t)segments_of((int)T) + 16);
    c->o_brank = a.take(4 * VCLOUD_MAX_HIST);
    hipError_t err = c->open(device, a.bytes);
    if (err == hipSuccess) err = c->pin(&c->h_io, 64 + 16 * T);
    if (err == hipSuccess) err = c->pin(&c->h_hdr, 4 * H_INTS);
    if (err == hipSuccess) err = hipMemsetAsync(c->d_mem, 0, 4 * H_INTS, c->stream);
    if (err == hipSuccess) err = hipMemsetAsync(c->d_mem + c->o_slotcnt, 0, 4 * (size_t)max_scans, c->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(c->stream);
    if (err != hipSuccess) { vcloud_destroy(c); VILCHK(err); }
    *out = c;
    return VIL_OK;
}

void vcloud_destroy(vcloud_ctx* c) {
    if (!c) return;
    c->close(c->prof);
    delete c;
}

int vcloud_reset(vcloud_ctx* c) {
    if (!c) return VIL_ERR_INVALID_ARGUMENT;
    c->head = 0; c->n_live = 0; c->n_cloud = 0;
    c->last_slot = -1; c->last_ds = c->last_view = c->last_fused = 0;
    return VIL_OK;
}

int vcloud_profile_enable(vcloud_ctx* c, int32_t enable) {
    if (!c) return VIL_ERR_INVALID_ARGUMENT;
    VILCHK(hipSetDevice(c->device));
    c->prof.on = enable != 0;
    return VIL_OK;
}
int vcloud_profile_read(vcloud_ctx* c, int64_t* launches10, double* total_ms10) {
    if (!c || !launches10 || !total_ms10) return VIL_ERR_INVALID_ARGUMENT;
    c->prof.read(launches10, total_ms10);
    return VIL_OK;
}

int vcloud_filter(vcloud_ctx* c, int32_t n, const float* xyzi, float leaf, int32_t hist_size, float* out_xyzi, int32_t capacity, int32_t* n_out) {
    if (!c || !n_out || n < 0 || (size_t)n > c->ntot || (n && !xyzi) || !finite_positive(leaf) || log2_of_hist(hist_size) < 0 || capacity < 0) return VIL_ERR_INVALID_ARGUMENT;
    VILCHK(hipSetDevice(c->device));
    int* hdr = c->at<int>(c->o_hdr);
    if (n) {
        memcpy(c->h_io, xyzi, 16 * (size_t)n);
        VILCHK(hipMemcpyAsync(c->d_mem + c->o_fin, c->h_io, 16 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    }
    VILCHK(hipMemsetD32Async((hipDeviceptr_t)(hdr + H_FIN), n, 1, c->stream));
    const int st = enqueue_filter(c, c->at<float4>(c->o_fin), hdr + H_FIN, n, leaf, hist_size, c->at<float4>(c->o_fout), hdr + H_FOUT);
    if (st != VIL_OK) return st;
    VILCHK(c->prof.mark(-1, 0, c->stream));
    VILCHK(hipMemcpyAsync(c->h_hdr, hdr, 4 * H_INTS, hipMemcpyDeviceToHost, c->stream));
    VILCHK(hipStreamSynchronize(c->stream));
    VILCHK(hipGetLastError());
    c->prof.collect();
    const int m = c->h_hdr[H_FOUT];
    if (m < 0 || m > n) return VIL_ERR_DEVICE;
    *n_out = m;
    if (capacity < m || (m && !out_xyzi)) return VIL_ERR_INVALID_ARGUMENT;
    if (m) {
        VILCHK(hipMemcpyAsync(c->h_io, c->d_mem + c->o_fout, 16 * (size_t)m, hipMemcpyDeviceToHost, c->stream));
        VILCHK(hipStreamSynchronize(c->stream));
        memcpy(out_xyzi, c->h_io, 16 * (size_t)m);
    }
    return VIL_OK;
}

int vcloud_push_scan(vcloud_ctx* c, double stamp, const float* lidar_to_world, int32_t n, const float* xyzi, const vcloud_options* opts, vcloud_summary* out) {
    vcloud_options o;
    vcloud_default_options(&o);
    if (opts) o = *opts;
    if (!c || !lidar_to_world || n < 0 || n > c->msp || (n && !xyzi) || !std::isfinite(stamp)) return VIL_ERR_INVALID_ARGUMENT;
    if (!finite_positive(o.leaf_scan) || !finite_positive(o.leaf_cloud) || log2_of_hist(o.hist_size) < 0 || std::isnan(o.max_coord) || std::isnan(o.max_ratio) || !(o.window_s >= 0.0))
        return VIL_ERR_INVALID_ARGUMENT;
    for (int k = 0; k < 12; ++k) if (!std::isfinite(lidar_to_world[k])) return VIL_ERR_INVALID_ARGUMENT;
    // step 4 on the host: the new scan is never popped (its own age is 0), so what the pop removes is decided by the stamps alone
    int popped = 0;
    while (popped < c->n_live && stamp - c->stamps[(c->head + popped) % c->ms] > o.window_s) ++popped;
    const int kept = c->n_live - popped;
    if (kept >= c->ms) return VIL_ERR_CAPACITY;
    const int head = (c->head + popped) % c->ms, slot = (head + kept) % c->ms, n_live = kept + 1;
    int fused_upper = n;
    for (int s = 0; s < kept; ++s) fused_upper += c->counts[(head + s) % c->ms];

    VILCHK(hipSetDevice(c->device));
    int* hdr = c->at<int>(c->o_hdr);
    const float* d_M = c->at<float>(c->o_up);
    const float4* d_raw = (const float4*)(c->d_mem + c->o_up + 64);
    float4* d_ds = c->at<float4>(c->o_ds); float4* d_slot = c->at<float4>(c->o_slots) + (size_t)slot * c->msp;
    int* d_flag = c->at<int>(c->o_evict);
    hipStream_t q = c->stream;
    const int nu = n > 0 ? n : 1, blocks = (nu + VC_BLK - 1) / VC_BLK;
    memcpy(c->h_io, lidar_to_world, 48);
    if (n) memcpy(c->h_io + 64, xyzi, 16 * (size_t)n);
    VILCHK(hipMemcpyAsync(c->d_mem + c->o_up, c->h_io, 64 + 16 * (size_t)n, hipMemcpyHostToDevice, q));
    VILCHK(hipMemsetD32Async((hipDeviceptr_t)(hdr + H_RAW), n, 1, q));
    int st = enqueue_filter(c, d_raw, hdr + H_RAW, n, o.leaf_scan, o.hist_size, d_ds, hdr + H_DS);                       // step 1
    if (st != VIL_OK) return st;
    VILCHK(c->prof.mark(K_VIEW, 1, q));
    hipLaunchKernelGGL(k_cloud_view, dim3(blocks), dim3(VC_BLK), 0, q, hdr + H_DS, nu, d_ds, o.max_coord, o.max_ratio, d_flag);   // step 2
    VILCHK(c->prof.mark(K_SCAN, 1, q));
    hipLaunchKernelGGL(k_cloud_scan, dim3(1), dim3(VC_SCAN), 0, q, d_flag, nu, hdr + H_VIEW);
    VILCHK(c->prof.mark(K_PLACE, 1, q));
    hipLaunchKernelGGL(k_cloud_place, dim3(blocks), dim3(VC_BLK), 0, q, hdr, nu, d_ds, d_flag, d_M, o.max_coord, o.max_ratio, d_slot, c->at<int>(c->o_slotcnt) + slot);   // step 3
    VILCHK(c->prof.mark(K_FUSE, 1, q));
    const int fu = fused_upper > 0 ? fused_upper : 1;
    hipLaunchKernelGGL(k_cloud_fuse, dim3((fu + VC_BLK - 1) / VC_BLK), dim3(VC_BLK), 0, q, hdr, fused_upper, head, n_live, c->ms, c->msp, c->at<int>(c->o_slotcnt),
                       c->at<float4>(c->o_slots), c->at<float4>(c->o_fused));                                                // step 5
    st = enqueue_filter(c, c->at<float4>(c->o_fused), hdr + H_FUSED, fused_upper, o.leaf_cloud, o.hist_size, c->at<float4>(c->o_cloud), hdr + H_CLOUD);   // step 6
    if (st != VIL_OK) return st;
    VILCHK(c->prof.mark(-1, 0, q));
    VILCHK(hipMemcpyAsync(c->h_hdr, hdr, 4 * H_INTS, hipMemcpyDeviceToHost, q));
    VILCHK(hipStreamSynchronize(q));                                                                                          // the one host wait
    VILCHK(hipGetLastError());
    c->prof.collect();
    const int* h = c->h_hdr;
    if (h[H_DS] < 0 || h[H_DS] > n || h[H_VIEW] < 0 || h[H_VIEW] > h[H_DS] || h[H_FUSED] < 0 || h[H_FUSED] > fused_upper || h[H_CLOUD] < 0 || h[H_CLOUD] > h[H_FUSED]) return VIL_ERR_DEVICE;
    // commit the queue
    c->head = head; c->n_live = n_live; c->stamps[slot] = stamp; c->counts[slot] = h[H_VIEW]; c->n_cloud = h[H_CLOUD];
    c->last_slot = slot; c->last_ds = h[H_DS]; c->last_view = h[H_VIEW]; c->last_fused = h[H_FUSED];
    if (out) {
        out->n_raw = n; out->n_scan_ds = h[H_DS]; out->n_in_view = h[H_VIEW]; out->n_scans = n_live; out->n_popped = popped; out->n_fused = h[H_FUSED]; out->n_cloud = h[H_CLOUD];
    }
    return VIL_OK;
}

int vcloud_read_cloud(vcloud_ctx* c, float* out_xyzi, int32_t capacity, int32_t* n) {
    if (!c) return VIL_ERR_INVALID_ARGUMENT;
    return read_points(c, c->o_cloud, c->n_cloud, out_xyzi, capacity, n);
}

int vcloud_debug_read(vcloud_ctx* c, int32_t stage, float* out_xyzi, int32_t capacity, int32_t* n) {
    if (!c) return VIL_ERR_INVALID_ARGUMENT;
    if (stage == VCLOUD_DBG_SCAN_DS) return read_points(c, c->o_ds, c->last_ds, out_xyzi, capacity, n);
    if (stage == VCLOUD_DBG_SCAN_WORLD) return read_points(c, c->o_slots + 16 * (size_t)(c->last_slot < 0 ? 0 : c->last_slot) * c->msp, c->last_view, out_xyzi, capacity, n);
    if (stage == VCLOUD_DBG_FUSED) return read_points(c, c->o_fused, c->last_fused, out_xyzi, capacity, n);
    return VIL_ERR_INVALID_ARGUMENT;
}

int vcloud_publish(vcloud_ctx* c, vdepth_ctx* depth) {
    if (!c || !depth) return VIL_ERR_INVALID_ARGUMENT;
    const vildepth_stage::Target t = vildepth_stage::target(depth);
    if (t.device != c->device) return VIL_ERR_INVALID_ARGUMENT;
    if (c->n_cloud > t.max_cloud_points) return VIL_ERR_CAPACITY;
    // every push ends with a wait on this context's stream: the cloud's writes are complete
    return vildepth_stage::replace_cloud(depth, c->n_cloud, c->at<float>(c->o_cloud), hipMemcpyDeviceToDevice);
}

}  // extern "C"
