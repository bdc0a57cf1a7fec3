// vilfeat.hip -- the device-resident feature tracker on gfx950 behind include/vilfeat.h (FeatureTracker::readImage as one call; the steps
// are numbered as in the header).
//
// The context owns a tracker, an epipolar and (cfg.equalize) a CLAHE context and drives their kernels through the hidden stage interfaces
// (viltrack_stage.hpp, vilepi_stage.hpp, vilclahe_stage.hpp): no kernel of those rows is defined twice.  Everything goes to the tracker's
// stream.  The point count of the moment lives in d_hdr[FH_N]; the stages' kernels read it and are launched over the host's upper bound.
// The kernels of this file are ONE workgroup of 1024 threads = 16 waves of 64 (the wave size is assumed in scan()): a thread owns 4
// adjacent points (1024 x 4 = VFEAT_MAX_POINTS_LIMIT), a compaction is an exclusive prefix sum of the threads' flag counts -- shuffles
// inside a wave, the 16 wave totals through LDS -- so the order of the survivors is the order of the points, whatever the timing.
//   k_feat_compact_lk    step 2's compaction on LK's status with step 3's increment; starts the device header of the call.
//   k_feat_records       step 4: the records of the hypotheses' counts (a prefix maximum), written to pinned host memory for the host's loop.
//   k_feat_compact_rank  step 4's compaction on the best hypothesis' inlier row (device memory; its index comes from the host), fused with
//                        step 5's priority order: the survivors' counts are staged in LDS and point k goes to the number of points that
//                        have a larger count or an equal one and a smaller index -- a stable sort by counting.
//   k_feat_compact_add   step 5's compaction on `kept` with addPoints.
//   k_feat_finish        steps 8-9: updateID as a prefix count over the -1s, the state for the next image, the message rows (a prefix count
//                        over track_cnt > 1) and the header, straight into pinned host memory.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/vilfeat.h"
#include "vil_host.hpp"
#include "vilclahe_stage.hpp"
#include "vilepi_stage.hpp"
#include "viltrack_stage.hpp"

#define VF_WG 1024
#define VF_PER 4                          // points of a thread: VF_WG * VF_PER == VFEAT_MAX_POINTS_LIMIT
static_assert(VF_WG * VF_PER == VFEAT_MAX_POINTS_LIMIT, "a thread of the one-workgroup kernels takes 4 points");

namespace {

// the device header (ints)
enum { FH_N = 0, FH_NTRACKED, FH_NINL, FH_NKEPT, FH_NCAND, FH_NNEW, FH_FAIL, FH_INTS = 16 };
// its mirror in pinned host memory (ints): [0] after LK, [1] after the hypotheses, the rest at the end
enum { HH_NTRACKED = 0, HH_NRECORDS, HH_N, HH_NROWS, HH_NEXT_ID, HH_NINL, HH_NKEPT, HH_NCAND, HH_NNEW, HH_FAIL, HH_INTS = 16 };
static_assert(4 * HH_INTS == VFEAT_HEADER_BYTES, "the header of vilfeat.h");

// exclusive prefix sum of v over the 1024 threads in thread order, and the total; every thread calls it (wave64: 16 waves)
__device__ __forceinline__ int scan(const int v, int* s_w, int& total) {
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int up = __shfl_up(incl, o); if (lane >= o) incl += up; }
    __syncthreads();                                                                                // the last call's reads of s_w are done
    if (lane == 63) s_w[w] = incl;
    __syncthreads();
    int base = 0; total = 0;
#pragma unroll
    for (int k = 0; k < VF_WG / 64; ++k) { const int x = s_w[k]; if (k < w) base += x; total += x; }
    return base + incl - v;
}

// the same with max in place of +, from `floor`
__device__ __forceinline__ int scan_max(const int v, int* s_w, const int floor) {
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int up = __shfl_up(incl, o); if (lane >= o) incl = max(incl, up); }
    __syncthreads();
    if (lane == 63) s_w[w] = incl;
    __syncthreads();
    int base = floor;
#pragma unroll
    for (int k = 0; k < VF_WG / 64; ++k) if (k < w) base = max(base, s_w[k]);
    const int before = __shfl_up(incl, 1);
    return lane ? max(base, before) : base;
}

// ---- steps 2-3 -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(VF_WG) void k_feat_compact_lk(int n, const uint8_t* __restrict__ status, const float2* __restrict__ cur_in, const float2* __restrict__ forw_in,
                                                           const int* __restrict__ ids_in, const int* __restrict__ cnt_in, float2* __restrict__ cur_out,
                                                           float2* __restrict__ forw_out, int* __restrict__ ids_out, int* __restrict__ cnt_out, int* __restrict__ hdr,
                                                           int* __restrict__ h_hdr) {
    __shared__ int s_w[VF_WG / 64];
    const int t = threadIdx.x, i0 = t * VF_PER;
    int f[VF_PER], mine = 0;
#pragma unroll
    for (int j = 0; j < VF_PER; ++j) { f[j] = i0 + j < n && status[i0 + j] ? 1 : 0; mine += f[j]; }           // n <= max_points <= 4096 (the host)
    int total, pos = scan(mine, s_w, total);
#pragma unroll
    for (int j = 0; j < VF_PER; ++j)
        if (f[j]) {                                                                                 // pos < total <= n
            const int i = i0 + j;
            cur_out[pos] = cur_in[i]; forw_out[pos] = forw_in[i]; ids_out[pos] = ids_in[i]; cnt_out[pos] = cnt_in[i] + 1;
            ++pos;
        }
    if (t < FH_INTS) hdr[t] = t == FH_N || t == FH_NTRACKED || t == FH_NINL ? total : 0;
    if (t == 0) h_hdr[HH_NTRACKED] = total;
}

// ---- step 4: the records ---------------------------------------------------------------------------------------------------------
// a thread takes `chunk` adjacent hypotheses; rec: pairs (h, count_h) in the order of h, at most n - 7 of them
__global__ __launch_bounds__(VF_WG) void k_feat_records(int max_iters, const int* __restrict__ counts, const int* __restrict__ hdr, int max_records, int* __restrict__ h_hdr,
                                                        int* __restrict__ rec) {
    __shared__ int s_w[VF_WG / 64];
    const int t = threadIdx.x;
    if (hdr[FH_N] < VEPI_SAMPLE) {                                                                  // the hypotheses did not run: uniform
        if (t == 0) h_hdr[HH_NRECORDS] = 0;
        return;
    }
    const int chunk = (max_iters + VF_WG - 1) / VF_WG, a = min(max_iters, t * chunk), b = min(max_iters, a + chunk);
    int m = VEPI_SAMPLE - 1;
    for (int h = a; h < b; ++h) m = max(m, counts[h]);
    const int before = scan_max(m, s_w, VEPI_SAMPLE - 1);                                           // the maximum of every earlier count, 7 at least
    int run = before, mine = 0;
    for (int h = a; h < b; ++h) { const int c = counts[h]; if (c > run) { run = c; ++mine; } }
    int total, pos = scan(mine, s_w, total);
    run = before;
    for (int h = a; h < b; ++h) {
        const int c = counts[h];
        if (c > run) {
            run = c;
            if (pos < max_records) { rec[2 * pos] = h; rec[2 * pos + 1] = c; }                    // counts rise strictly from 8 to n at most: total <= n - 7
            ++pos;
        }
    }
    if (t == 0) h_hdr[HH_NRECORDS] = min(total, max_records);
}

// ---- step 4's compaction and step 5's priority order -----------------------------------------------------------------------------
__global__ __launch_bounds__(VF_WG) void k_feat_compact_rank(int best_h, const unsigned long long* __restrict__ bits, int stride, const float2* __restrict__ forw_in,
                                                             const int* __restrict__ ids_in, const int* __restrict__ cnt_in, float2* __restrict__ forw_out,
                                                             int* __restrict__ ids_out, int* __restrict__ cnt_out, int* __restrict__ hdr) {
    __shared__ int s_w[VF_WG / 64];
    __shared__ int s_cnt[VFEAT_MAX_POINTS_LIMIT], s_src[VFEAT_MAX_POINTS_LIMIT];
    const int t = threadIdx.x, i0 = t * VF_PER, n = hdr[FH_N];
    unsigned long long word = ~0ull;
    if (best_h >= 0 && i0 < n) word = bits[(size_t)best_h * stride + (i0 >> 6)];                    // the 4 points of a thread share a word; i0 / 64 < ceil(n / 64) <= stride
    int f[VF_PER], mine = 0;
#pragma unroll
    for (int j = 0; j < VF_PER; ++j) { f[j] = i0 + j < n ? (int)((word >> ((i0 + j) & 63)) & 1) : 0; mine += f[j]; }
    int m, pos = scan(mine, s_w, m);
#pragma unroll
    for (int j = 0; j < VF_PER; ++j)
        if (f[j]) { s_cnt[pos] = cnt_in[i0 + j]; s_src[pos] = i0 + j; ++pos; }                      // pos < m <= n <= 4096
    __syncthreads();
    for (int k = t; k < m; k += VF_WG) {
        const int c = s_cnt[k];
        int rank = 0;
        for (int j = 0; j < m; ++j) { const int cj = s_cnt[j]; rank += cj > c || (cj == c && j < k) ? 1 : 0; }       // a permutation of 0 .. m - 1
        const int src = s_src[k];
        forw_out[rank] = forw_in[src]; ids_out[rank] = ids_in[src]; cnt_out[rank] = c;
    }
    if (t == 0) { hdr[FH_N] = m; hdr[FH_NINL] = m; }
}

// ---- step 5's compaction and addPoints -------------------------------------------------------------------------------------------
// thdr, kept, new_xy: what the tracker's detection left (viltrack_stage::Detection)
__global__ __launch_bounds__(VF_WG) void k_feat_compact_add(const uint8_t* __restrict__ kept, const int* __restrict__ thdr, const float2* __restrict__ new_xy, int max_cand,
                                                            int capacity, const float2* __restrict__ forw_in, const int* __restrict__ ids_in, const int* __restrict__ cnt_in,
                                                            float2* __restrict__ pts_out, int* __restrict__ ids_out, int* __restrict__ cnt_out, int* __restrict__ hdr) {
    __shared__ int s_w[VF_WG / 64];
    const int t = threadIdx.x, i0 = t * VF_PER, n = hdr[FH_N];
    int f[VF_PER], mine = 0;
#pragma unroll
    for (int j = 0; j < VF_PER; ++j) { f[j] = i0 + j < n && kept[i0 + j] ? 1 : 0; mine += f[j]; }
    int nk, pos = scan(mine, s_w, nk);
#pragma unroll
    for (int j = 0; j < VF_PER; ++j)
        if (f[j]) { const int i = i0 + j; pts_out[pos] = forw_in[i]; ids_out[pos] = ids_in[i]; cnt_out[pos] = cnt_in[i]; ++pos; }
    const int ncand = thdr[viltrack_stage::H_NCAND];
    const int nn = ncand > max_cand ? 0 : min(thdr[viltrack_stage::H_NNEW], capacity - nk);        // nk + nn <= max_cnt by step 10; the min is the bound of the arrays
    for (int k = t; k < nn; k += VF_WG) { pts_out[nk + k] = new_xy[k]; ids_out[nk + k] = -1; cnt_out[nk + k] = 1; }
    if (t == 0) {
        hdr[FH_N] = nk + max(nn, 0); hdr[FH_NKEPT] = nk; hdr[FH_NNEW] = max(nn, 0); hdr[FH_NCAND] = ncand;
        hdr[FH_FAIL] = thdr[viltrack_stage::H_FAIL];
    }
}

// ---- steps 8-9 -------------------------------------------------------------------------------------------------------------------
struct Msg { float *xyz, *id, *u, *v, *vx, *vy; };

__global__ __launch_bounds__(VF_WG) void k_feat_finish(int next_id, int publish, const float2* __restrict__ pts_in, const int* __restrict__ ids_in, const int* __restrict__ cnt_in,
                                                       const float2* __restrict__ un, const float2* __restrict__ vel, float2* __restrict__ pts_out, int* __restrict__ ids_out,
                                                       int* __restrict__ cnt_out, const Msg msg, const int* __restrict__ hdr, int* __restrict__ h_hdr) {
    __shared__ int s_w[VF_WG / 64];
    const int t = threadIdx.x, i0 = t * VF_PER, n = hdr[FH_N];
    int id[VF_PER], cnt[VF_PER], fresh = 0, rows = 0;
#pragma unroll
    for (int j = 0; j < VF_PER; ++j) {
        const bool in = i0 + j < n;
        id[j] = in ? ids_in[i0 + j] : 0; cnt[j] = in ? cnt_in[i0 + j] : 0;
        fresh += in && id[j] == -1 ? 1 : 0; rows += publish && cnt[j] > 1 ? 1 : 0;
    }
    int n_fresh, n_rows, nid = next_id + scan(fresh, s_w, n_fresh), row = scan(rows, s_w, n_rows);
#pragma unroll
    for (int j = 0; j < VF_PER; ++j) {
        const int i = i0 + j;
        if (i >= n) break;
        if (id[j] == -1) id[j] = nid++;                                                             // step 8
        const float2 p = pts_in[i];
        pts_out[i] = p; ids_out[i] = id[j]; cnt_out[i] = cnt[j];
        if (publish && cnt[j] > 1) {                                                                // step 9; row < n_rows <= n <= max_cnt, the room of the message
            const float2 q = un[i], w = vel[i];
            msg.xyz[3 * row] = q.x; msg.xyz[3 * row + 1] = q.y; msg.xyz[3 * row + 2] = 1.0f;
            msg.id[row] = (float)id[j]; msg.u[row] = p.x; msg.v[row] = p.y; msg.vx[row] = w.x; msg.vy[row] = w.y;
            ++row;
        }
    }
    if (t == 0) {
        h_hdr[HH_N] = n; h_hdr[HH_NROWS] = n_rows; h_hdr[HH_NEXT_ID] = next_id + n_fresh; h_hdr[HH_NINL] = hdr[FH_NINL]; h_hdr[HH_NKEPT] = hdr[FH_NKEPT];
        h_hdr[HH_NCAND] = hdr[FH_NCAND]; h_hdr[HH_NNEW] = hdr[FH_NNEW]; h_hdr[HH_FAIL] = hdr[FH_FAIL];
    }
}

struct PointSet { float2 *cur, *forw; int *ids, *cnt; };

}  // namespace

struct vfeat_ctx {                           // d_mem: header | sets A, B (cur, forw, ids, cnt) | LK's forw, status | un, vel | table 0 | table 1
    vfeat_cfg cfg = {};
    int device = -1;                         // -1: nothing of its own to free
    char* d_mem = nullptr;
    vtrack_ctx* trk = nullptr; vepi_ctx* epi = nullptr; vclahe_ctx* clahe = nullptr;
    hipStream_t q = nullptr;                 // the tracker's stream: every launch of a call goes there
    int* d_hdr = nullptr; PointSet A = {}, B = {};          // the state between calls is A.cur, A.ids, A.cnt
    float2* d_lkforw = nullptr; uint8_t* d_status = nullptr; float2* d_un = nullptr; float2* d_vel = nullptr;
    int* d_tab_ids[2] = {}; float2* d_tab_un[2] = {};
    char* h_pin = nullptr; int* h_hdr = nullptr; int* h_rec = nullptr; float* h_msg = nullptr;     // pinned: header | records | message; the kernels' views of them:
    int* k_hdr = nullptr; int* k_rec = nullptr; float* k_msg = nullptr;
    int n = 0, next_id = 0, tab = 0;         // points now (also the length of table `tab`), the next id, the slot of the previous table
    double prev_time = 0.0;
    int waits = 0; int64_t up = 0, down = 0; // of the call that runs
    vilhost::Profiler<VFEAT_NUM_KERNELS, 2 * VFEAT_NUM_KERNELS> prof;
};

// the single place where the row waits, and the single place where it copies
static hipError_t wait(vfeat_ctx* c) {
    c->waits++;
    const hipError_t e = hipStreamSynchronize(c->q);
    return e != hipSuccess ? e : hipGetLastError();
}
static hipError_t copy_up(vfeat_ctx* c, void* dst, const void* src, size_t bytes) {
    c->up += (int64_t)bytes;
    return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->q);
}

static void forget(vfeat_ctx* c) {
    c->n = 0; c->prev_time = 0.0;
    viltrack_stage::forget(c->trk);
}

struct Ransac { int found = 0, best_h = -1, consumed = 0, n_records = 0; };

// steps 1-9, up to the last wait.  A VIL_* status; anything but VIL_OK leaves the context to be forgotten by the caller.
static int run(vfeat_ctx* c, const uint8_t* gray, const int row_stride, const double time_s, const int publish, const uint64_t seed, Ransac& r) {
    const vfeat_cfg& g = c->cfg;
    const size_t WH = (size_t)g.width * g.height;
    const viltrack_stage::Target tg = viltrack_stage::target(c->trk);
    int st;
    if (g.equalize) {                                                                               // step 1
        const vilclahe_stage::Staged s = vilclahe_stage::stage_image(c->clahe, gray, row_stride);
        VILCHK(copy_up(c, s.dev, s.host, WH));
        if ((st = vilclahe_stage::enqueue_kernels(c->clahe, c->q, tg.level0, nullptr)) != VIL_OK) return st;
    } else {
        VILCHK(copy_up(c, tg.level0, viltrack_stage::stage_image(c->trk, gray, row_stride), WH));
    }
    if ((st = viltrack_stage::enqueue_push(c->trk)) != VIL_OK) return st;
    viltrack_stage::commit_push(c->trk);
    const int n0 = c->n;
    const PointSet &A = c->A, &B = c->B;
    if (n0 && (st = viltrack_stage::enqueue_lk(c->trk, n0, nullptr, (const float*)A.cur, (float*)c->d_lkforw, c->d_status)) != VIL_OK) return st;      // step 2
    VILCHK(c->prof.mark(0, c->q));
    hipLaunchKernelGGL(k_feat_compact_lk, dim3(1), dim3(VF_WG), 0, c->q, n0, c->d_status, A.cur, c->d_lkforw, A.ids, A.cnt, B.cur, B.forw, B.ids, B.cnt, c->d_hdr, c->k_hdr);
    VILCHK(c->prof.mark(1, c->q));
    c->down += 4;
    const bool ransac = publish && n0 >= VEPI_SAMPLE;                                               // the device skips it when n_tracked < 8
    if (ransac) {                                                                                   // step 4
        const vilepi_stage::Buffers eb = vilepi_stage::buffers(c->epi);
        vilepi_stage::lift(c->epi, c->q, n0, c->d_hdr + FH_N, B.cur, B.forw, eb.p1, eb.p2);
        vilepi_stage::hypotheses(c->epi, c->q, n0, c->d_hdr + FH_N, 0, g.max_iters, seed, g.f_threshold * g.f_threshold, eb, eb.counts, eb.bits);
        VILCHK(c->prof.mark(2, c->q));
        hipLaunchKernelGGL(k_feat_records, dim3(1), dim3(VF_WG), 0, c->q, g.max_iters, eb.counts, c->d_hdr, g.max_points, c->k_hdr, c->k_rec);
        VILCHK(c->prof.mark(3, c->q));
        VILCHK(wait(c));
        const int n = c->h_hdr[HH_NTRACKED];
        r.n_records = c->h_hdr[HH_NRECORDS];
        c->down += 4 + 8 * (int64_t)r.n_records;
        if (n >= VEPI_SAMPLE) {                                                                     // vilepi.h step 6 over the records
            int niters = g.max_iters, last = -1;
            for (int k = 0; k < r.n_records; ++k) {
                const int h = c->h_rec[2 * k], count = c->h_rec[2 * k + 1];
                if (h >= niters) break;                                                             // the loop ended before it
                r.best_h = h; last = h;
                niters = std::min(niters, vilepi_stage::update_iters(g.confidence, (double)(n - count) / (double)n, g.max_iters));
            }
            r.consumed = std::max(niters, last + 1);
            r.found = r.best_h >= 0;
        }
    }
    int n_max = n0;
    if (publish) {                                                                                  // step 5
        const vilepi_stage::Buffers eb = vilepi_stage::buffers(c->epi);
        VILCHK(c->prof.mark(4, c->q));
        hipLaunchKernelGGL(k_feat_compact_rank, dim3(1), dim3(VF_WG), 0, c->q, r.best_h, (const unsigned long long*)eb.bits, eb.words, B.forw, B.ids, B.cnt, A.forw, A.ids,
                           A.cnt, c->d_hdr);
        VILCHK(c->prof.mark(5, c->q));
        viltrack_stage::Detection det;
        if ((st = viltrack_stage::enqueue_detect(c->trk, n0, c->d_hdr + FH_N, (const float*)A.forw, g.min_dist, g.max_cnt, g.quality, &det)) != VIL_OK) return st;
        VILCHK(c->prof.mark(6, c->q));
        hipLaunchKernelGGL(k_feat_compact_add, dim3(1), dim3(VF_WG), 0, c->q, det.kept, det.hdr, (const float2*)det.new_xy, g.max_candidates, g.max_points, A.forw, A.ids, A.cnt,
                           B.forw, B.ids, B.cnt, c->d_hdr);
        VILCHK(c->prof.mark(7, c->q));
        n_max = g.max_cnt;                                                                          // n_kept <= n0 <= max_cnt, and the picks fill up to max_cnt
    }
    const int nt = 1 - c->tab;                                                                      // steps 6-7: the points of the image are B.forw either way
    if (n_max)
        vilepi_stage::undistort(c->epi, c->q, n_max, c->d_hdr + FH_N, B.forw, B.ids, time_s - c->prev_time, c->n, c->d_tab_ids[c->tab], c->d_tab_un[c->tab], c->d_tab_ids[nt],
                                c->d_tab_un[nt], c->d_un, c->d_vel);
    const int M = g.max_cnt;
    const Msg km = {c->k_msg, c->k_msg + 3 * M, c->k_msg + 4 * M, c->k_msg + 5 * M, c->k_msg + 6 * M, c->k_msg + 7 * M};
    VILCHK(c->prof.mark(8, c->q));
    hipLaunchKernelGGL(k_feat_finish, dim3(1), dim3(VF_WG), 0, c->q, c->next_id, publish, B.forw, B.ids, B.cnt, c->d_un, c->d_vel, A.cur, A.ids, A.cnt, km, c->d_hdr, c->k_hdr);
    VILCHK(c->prof.mark(9, c->q));
    VILCHK(wait(c));
    c->prof.span(0, 0, 1);
    if (ransac) c->prof.span(1, 2, 3);
    if (publish) { c->prof.span(2, 4, 5); c->prof.span(3, 6, 7); }
    c->prof.span(4, 8, 9);
    const int* h = c->h_hdr;
    c->down += 4 * (HH_INTS - 2) + VFEAT_ROW_BYTES * (int64_t)h[HH_NROWS];
    if (h[HH_FAIL]) return VIL_ERR_DEVICE;
    if (h[HH_NCAND] > g.max_candidates) return VIL_ERR_UNSUPPORTED;
    if (n_max) c->tab = nt;
    c->n = h[HH_N]; c->next_id = h[HH_NEXT_ID]; c->prev_time = time_s;
    return VIL_OK;
}

extern "C" {

void vfeat_destroy(vfeat_ctx* c) {
    if (!c) return;
    if (c->device >= 0) {
        hipSetDevice(c->device);
        if (c->d_mem) hipFree(c->d_mem);
        if (c->h_pin) hipHostFree(c->h_pin);
        c->prof.destroy();
    }
    vclahe_destroy(c->clahe); vepi_destroy(c->epi); vtrack_destroy(c->trk);                          // the stream is the tracker's
    delete c;
}

int vfeat_create(int32_t device, const vfeat_cfg* g, vfeat_ctx** out) {
    if (!out || !g) return VIL_ERR_INVALID_ARGUMENT;
    const double cam[9] = {g->fx, g->fy, g->cx, g->cy, g->k1, g->k2, g->p1, g->p2, g->focal};
    for (const double v : cam) if (!std::isfinite(v)) return VIL_ERR_INVALID_ARGUMENT;
    if (g->fx == 0.0 || g->fy == 0.0 || g->width < 16 || g->width > 16384 || g->height < 16 || g->height > 16384 || g->max_level < 0 || g->max_level > VTRACK_MAX_LEVEL ||
        g->max_points < VFEAT_MIN_POINTS_LIMIT || g->max_points > VFEAT_MAX_POINTS_LIMIT || g->max_candidates < 1 || g->model < VEPI_MODEL_PINHOLE ||
        g->model > VEPI_MODEL_SCARAMUZZA || g->max_iters < 1 || g->max_iters > VEPI_MAX_ITERS_LIMIT || (g->equalize != 0 && g->equalize != 1) ||
        (g->equalize && (g->tiles_x < 1 || g->tiles_x > VCLAHE_MAX_TILES || g->tiles_y < 1 || g->tiles_y > VCLAHE_MAX_TILES || !std::isfinite(g->clip_limit) ||
                         g->clip_limit < 0.0)) ||
        g->max_cnt < 1 || g->max_cnt > g->max_points || g->min_dist < 0 || g->min_dist > VTRACK_MAX_MIN_DIST || !(g->quality > 0.0f && g->quality <= 1.0f) ||
        !(g->f_threshold > 0.0) || !std::isfinite(g->f_threshold) || !(g->confidence > 0.0 && g->confidence < 1.0))
        return VIL_ERR_INVALID_ARGUMENT;
    if (g->model != VEPI_MODEL_PINHOLE) return VIL_ERR_UNSUPPORTED;
    vfeat_ctx* c = new vfeat_ctx();
    c->cfg = *g;
    const vtrack_cfg tc = {g->width, g->height, g->max_level, g->max_points, g->max_candidates};
    vepi_cfg ec = {};
    ec.fx = g->fx; ec.fy = g->fy; ec.cx = g->cx; ec.cy = g->cy; ec.k1 = g->k1; ec.k2 = g->k2; ec.p1 = g->p1; ec.p2 = g->p2; ec.focal = g->focal;
    ec.width = g->width; ec.height = g->height; ec.model = g->model; ec.max_points = g->max_points; ec.max_iters = g->max_iters;
    ec.readback = VEPI_READBACK_COPY;                                                              // the counts and the inlier rows stay in its device arena
    int st = vtrack_create(device, &tc, &c->trk);
    if (st == VIL_OK) st = vepi_create(device, &ec, &c->epi);
    if (st == VIL_OK && g->equalize) {
        const vclahe_cfg cc = {g->width, g->height, g->tiles_x, g->tiles_y, g->clip_limit};
        st = vclahe_create(device, &cc, &c->clahe);
    }
    if (st != VIL_OK) { vfeat_destroy(c); return st; }
    c->device = device;
    c->q = viltrack_stage::target(c->trk).stream;
    const size_t P = (size_t)g->max_points, M = (size_t)g->max_cnt;
    vilhost::Arena a;
    const size_t o_hdr = a.take(4 * FH_INTS);
    size_t o_set[2][4];
    for (auto& s : o_set) { s[0] = a.take(8 * P); s[1] = a.take(8 * P); s[2] = a.take(4 * P); s[3] = a.take(4 * P); }
    const size_t o_lkforw = a.take(8 * P), o_status = a.take(P), o_un = a.take(8 * P), o_vel = a.take(8 * P);
    const size_t o_tab[2][2] = {{a.take(4 * P), a.take(8 * P)}, {a.take(4 * P), a.take(8 * P)}};
    const size_t p_rec = 4 * HH_INTS, p_msg = p_rec + vilhost::up16(8 * P), p_bytes = p_msg + vilhost::up16(VFEAT_ROW_BYTES * M);
    hipError_t err = hipSetDevice(device);
    if (err == hipSuccess) err = hipMalloc(&c->d_mem, a.bytes);
    if (err == hipSuccess) err = hipHostMalloc((void**)&c->h_pin, p_bytes, hipHostMallocDefault);
    void* dev = nullptr;
    if (err == hipSuccess) err = hipHostGetDevicePointer(&dev, c->h_pin, 0);
    if (err == hipSuccess) err = hipMemsetAsync(c->d_mem, 0, a.bytes, c->q);
    if (err == hipSuccess) err = hipStreamSynchronize(c->q);
    if (err != hipSuccess) { vfeat_destroy(c); VILCHK(err); }
    memset(c->h_pin, 0, p_bytes);
    char* d = c->d_mem;
    c->d_hdr = (int*)(d + o_hdr);
    PointSet* sets[2] = {&c->A, &c->B};
    for (int k = 0; k < 2; ++k) *sets[k] = {(float2*)(d + o_set[k][0]), (float2*)(d + o_set[k][1]), (int*)(d + o_set[k][2]), (int*)(d + o_set[k][3])};
    c->d_lkforw = (float2*)(d + o_lkforw); c->d_status = (uint8_t*)(d + o_status); c->d_un = (float2*)(d + o_un); c->d_vel = (float2*)(d + o_vel);
    for (int k = 0; k < 2; ++k) { c->d_tab_ids[k] = (int*)(d + o_tab[k][0]); c->d_tab_un[k] = (float2*)(d + o_tab[k][1]); }
    c->h_hdr = (int*)c->h_pin; c->h_rec = (int*)(c->h_pin + p_rec); c->h_msg = (float*)(c->h_pin + p_msg);
    c->k_hdr = (int*)dev; c->k_rec = (int*)((char*)dev + p_rec); c->k_msg = (float*)((char*)dev + p_msg);
    *out = c;
    return VIL_OK;
}

int vfeat_profile_enable(vfeat_ctx* c, int32_t enable) {
    if (!c) return VIL_ERR_INVALID_ARGUMENT;
    VILCHK(c->prof.enable(c->device, enable != 0));
    return VIL_OK;
}
int vfeat_profile_read(vfeat_ctx* c, int64_t* launches5, double* total_ms5) {
    if (!c || !launches5 || !total_ms5) return VIL_ERR_INVALID_ARGUMENT;
    c->prof.read(launches5, total_ms5);
    return VIL_OK;
}

int vfeat_read_image(vfeat_ctx* c, const uint8_t* gray, int32_t row_stride, double time_s, int32_t publish, uint64_t seed, vfeat_msg* msg, vfeat_summary* out) {
    if (!c || !gray || row_stride < c->cfg.width || std::isnan(time_s) ||
        (publish && (!msg || !msg->points_xyz || !msg->id || !msg->u || !msg->v || !msg->vx || !msg->vy)))
        return VIL_ERR_INVALID_ARGUMENT;
    VILCHK(hipSetDevice(c->device));
    c->waits = 0; c->up = c->down = 0;
    const int n_before = c->n;
    Ransac r;
    const int st = run(c, gray, row_stride, time_s, publish ? 1 : 0, seed, r);
    if (st != VIL_OK) {                                                                             // no output; as after vfeat_reset
        hipStreamSynchronize(c->q);
        forget(c);
        return st;
    }
    const int* h = c->h_hdr;
    const int rows = h[HH_NROWS], M = c->cfg.max_cnt;
    if (publish) {
        float* dst[6] = {msg->points_xyz, msg->id, msg->u, msg->v, msg->vx, msg->vy};
        for (int k = 0; k < 6; ++k) if (rows) memcpy(dst[k], c->h_msg + (k ? (2 + k) * M : 0), 4 * (size_t)rows * (k ? 1 : 3));
    }
    if (msg) msg->n_rows = rows;
    if (out) {
        memset(out, 0, sizeof *out);
        out->n_before = n_before; out->n_tracked = h[HH_NTRACKED]; out->n_inliers = h[HH_NINL];
        out->found = r.found; out->best_hypothesis = r.best_h; out->consumed = r.consumed; out->n_records = r.n_records;
        out->n_kept = h[HH_NKEPT]; out->n_candidates = h[HH_NCAND]; out->n_new = h[HH_NNEW];
        out->n = h[HH_N]; out->n_rows = rows; out->next_id = h[HH_NEXT_ID];
        out->host_waits = c->waits; out->bytes_up = c->up; out->bytes_down = c->down;
    }
    return VIL_OK;
}

int vfeat_reset(vfeat_ctx* c) {
    if (!c) return VIL_ERR_INVALID_ARGUMENT;
    forget(c);
    return VIL_OK;
}

int vfeat_debug_read(vfeat_ctx* c, int32_t what, int32_t arg, void* dst, int64_t capacity_bytes) {
    if (!c || !dst) return VIL_ERR_INVALID_ARGUMENT;
    if (what == VFEAT_DBG_CUR_LEVEL || what == VFEAT_DBG_FORW_LEVEL)
        return vtrack_debug_read(c->trk, what == VFEAT_DBG_CUR_LEVEL ? VTRACK_DBG_CUR_LEVEL : VTRACK_DBG_FORW_LEVEL, arg, dst, capacity_bytes);
    const size_t n = (size_t)c->n;
    char* o = (char*)dst;
    if (what == VFEAT_DBG_STATE) {
        if (capacity_bytes < (int64_t)(4 + 16 * n)) return VIL_ERR_INVALID_ARGUMENT;
        const int32_t n32 = c->n;
        memcpy(o, &n32, 4);
        if (!n) return VIL_OK;
        VILCHK(hipSetDevice(c->device));
        VILCHK(hipMemcpyAsync(o + 4, c->A.cur, 8 * n, hipMemcpyDeviceToHost, c->q));
        VILCHK(hipMemcpyAsync(o + 4 + 8 * n, c->A.ids, 4 * n, hipMemcpyDeviceToHost, c->q));
        VILCHK(hipMemcpyAsync(o + 4 + 12 * n, c->A.cnt, 4 * n, hipMemcpyDeviceToHost, c->q));
    } else if (what == VFEAT_DBG_UN_VEL) {
        if (capacity_bytes < (int64_t)(16 * n)) return VIL_ERR_INVALID_ARGUMENT;
        if (!n) return VIL_OK;
        VILCHK(hipSetDevice(c->device));
        VILCHK(hipMemcpyAsync(o, c->d_un, 8 * n, hipMemcpyDeviceToHost, c->q));
        VILCHK(hipMemcpyAsync(o + 8 * n, c->d_vel, 8 * n, hipMemcpyDeviceToHost, c->q));
    } else {
        return VIL_ERR_INVALID_ARGUMENT;
    }
    VILCHK(hipStreamSynchronize(c->q));
    return VIL_OK;
}

}  // extern "C"
