// villmap.hip -- lidar_mapping's local cube map, resident on gfx950, behind include/villmap.h (lidar_mapping/src/localMapping.cpp:
// process() :338-982; the steps are numbered as in the header).
//
// WHERE THINGS LIVE.  A class's cubes are pieces of one pool of max_map_points points; a table on the HOST says where each cube starts
// and how many points it holds (2 x 847 pairs of ints).  The host knows t_w_curr before any device work, so the shifts of step 2 are
// moves of table entries and no point moves.  Every push uploads the table and writes the cubes into the OTHER pool of the pair; the
// table that comes back with the counts is committed when the call has succeeded, so a refused or failed call changes nothing.
//   k_lmap_gather    step 3: a workgroup per valid cube and class copies the cube behind its predecessors (offsets from the host).
//   (filter A)       step 4: vilcloud_stage::filter_resident twice on the private vcloud_ctx's stream, between two events.
//   (registration)   step 5: vilmap_stage::set_map_resident and align_resident on the private vmap_ctx.
//   k_lmap_place     step 6: a thread per stack point: pointAssociateToMap and the cube of the float point (-1: dropped).
//   k_lmap_layout    ONE workgroup: how many points every cube receives (integer counts in LDS: no order in them), and the exclusive
//                    sum of old + received over the cubes: where every cube starts in the new pool.
//   k_lmap_append    a workgroup per cube and class: the old points, then the received ones in stack order -- it walks the class's
//                    cube numbers 256 at a time, ballots and popcounts give the rank.  A stable scatter without a sort: 847 workgroups
//                    read a few thousand ints each.
//   k_lmap_refilter  step 7, the segmented filter A: a workgroup per VALID cube and class runs the whole of filter A on its own cube
//                    -- voxels, the stable counting sort by table entry (the four waves take a quarter of the cube each, histograms in
//                    LDS), run starts, the scan of the eviction flags, the sequential sums -- with the device functions vilcloud.hip
//                    runs (vilcloud_dev.hpp).  Its table entries are its own LDS: two cubes cannot see each other's.  Any cube length
//                    up to the pool takes this one path; the work arrays are global memory at the cube's own place.
//   k_lmap_publish   step 8: a workgroup per cube: corner then surf, behind the cubes before it; the world and the sensor frame.
// The grids of all six are fixed (75 x 2, 847 x 2, 1, or the number of stack points): the number of launches of a push does not depend
// on which cubes hold points.  No kernel waits for another workgroup; the only atomics are integer counts in LDS.
// HOST WAITS per push: one for the stacks' counts (the registration's grids are sized by them), those of vmap_set_map / vmap_align
// themselves, one at the end for the table.
// The arithmetic of the contract is kept unfused and in source order (hipcc would contract a * b + c), on the host too:
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/villmap.h"
#include "vil_host.hpp"
#include "vilcloud_dev.hpp"
#include "vilcloud_stage.hpp"
#include "vilmap_stage.hpp"

#define LM_BLK 256
#define LM_WAVES (LM_BLK / 64)
#define LM_ONE 1024                          // threads of k_lmap_layout
#define LM_CUBES VLMAP_CUBES
#define LM_MAX_POINTS (1 << 24)

namespace {
using namespace vilcloud_dev;

enum { K_GATHER = 0, K_PLACE, K_LAYOUT, K_APPEND, K_REFILTER, K_PUBLISH };
static_assert(K_PUBLISH + 1 == VLMAP_NUM_KERNELS, "one profile entry per kernel");
// what goes up per push (ints): the table, the valid cubes (-1: none) and where each starts in the from-map cloud
enum { U_START = 0, U_COUNT = 2 * LM_CUBES, U_VALID = 4 * LM_CUBES, U_FMOFF = U_VALID + 76, U_INTS = U_FMOFF + 2 * 76 };
// what comes down (ints): the header, the matrix step 6 used (12 doubles), the new table
enum { H_RAW = 0, H_STACK = 2, H_ADDED = 4, D_MATRIX = 16, D_START = D_MATRIX + 24, D_COUNT = D_START + 2 * LM_CUBES, D_INTS = D_COUNT + 2 * LM_CUBES };
static_assert(U_INTS % 4 == 0 && D_INTS % 2 == 0, "alignment of what follows");

struct Mat34 { double m[12]; };              // R row-major (9), then t (3): the layout of vp1::PoseRT
struct Geo { int cen[3]; double len, hgt; };

// the exclusive sum of v over the NW waves of the workgroup, and the sum; two barriers, so s_w can be used again at once
template <int NW>
__device__ __forceinline__ int block_exclusive(const int v, int* s_w, int& all) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
    for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(inc, o); if (lane >= o) inc += u; }
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    int before = 0; all = 0;
    for (int w = 0; w < NW; ++w) { const int c = s_w[w]; before += w < wave ? c : 0; all += c; }
    __syncthreads();
    return before + inc - v;
}

// steps 2 and 6: the cube along one axis.  H = 0.0 (the QUIRK): double division, truncation, decrement when negative.
__host__ __device__ __forceinline__ int cube_of(const double v, const double size, const int cen) {
    const double s = v + 0.0;
    const double qd = s / size;
    if (!(qd > -1.0e6 && qd < 1.0e6)) return -(1 << 20);                                          // far outside any array (and NaN): no int overflow
    int c = (int)qd + cen;
    if (s < 0.0) --c;
    return c;
}

// step 3: valid cube v of class y, behind the valid cubes before it
__global__ __launch_bounds__(LM_BLK) void k_lmap_gather(const int* __restrict__ up, int maxmap, const float4* __restrict__ pool, int fm_cap, float4* __restrict__ fm) {
    const int cls = blockIdx.y, c = up[U_VALID + blockIdx.x];
    if (c < 0) return;
    const int e = cls * LM_CUBES + c, n = up[U_COUNT + e], dst = up[U_FMOFF + cls * 76 + blockIdx.x];
    const float4* src = pool + (size_t)cls * maxmap + up[U_START + e];
    float4* out = fm + (size_t)cls * fm_cap + dst;                                                // dst + n <= the class's points <= fm_cap: the host summed the same counts
    for (int i = threadIdx.x; i < n; i += LM_BLK) out[i] = src[i];
}

// step 6: stack point g (corner points first) -> the map-frame float point and its cube; thread 0 leaves the matrix it used
__global__ __launch_bounds__(LM_BLK) void k_lmap_place(int n_c, int n_s, int msp, const float4* __restrict__ stack, Mat34 M, const double* __restrict__ Mdev, Geo G, float4* __restrict__ placed,
                                                       int* __restrict__ cube, double* __restrict__ used) {
    const int g = blockIdx.x * LM_BLK + threadIdx.x;
    if (Mdev) for (int k = 0; k < 12; ++k) M.m[k] = Mdev[k];                                        // both hold R (9, row-major) then t (3), as vp1::PoseRT
    if (g == 0) for (int r = 0; r < 3; ++r) { used[4 * r] = M.m[3 * r]; used[4 * r + 1] = M.m[3 * r + 1]; used[4 * r + 2] = M.m[3 * r + 2]; used[4 * r + 3] = M.m[9 + r]; }
    if (g >= n_c + n_s) return;
    const int cls = g >= n_c ? 1 : 0, i = g - (cls ? n_c : 0);
    const float4 p = stack[(size_t)cls * msp + i];
    const double x = p.x, y = p.y, z = p.z;
    const float fx = (float)(((M.m[0] * x + M.m[1] * y) + M.m[2] * z) + M.m[9]);
    const float fy = (float)(((M.m[3] * x + M.m[4] * y) + M.m[5] * z) + M.m[10]);
    const float fz = (float)(((M.m[6] * x + M.m[7] * y) + M.m[8] * z) + M.m[11]);
    int c = -1;
    if (isfinite(fx) && isfinite(fy) && isfinite(fz)) {                                             // the DEVIATION
        const int ci = cube_of((double)fx, G.len, G.cen[0]), cj = cube_of((double)fy, G.len, G.cen[1]), ck = cube_of((double)fz, G.hgt, G.cen[2]);
        if (ci >= 0 && ci < VLMAP_W && cj >= 0 && cj < VLMAP_H && ck >= 0 && ck < VLMAP_D) c = ci + VLMAP_W * cj + VLMAP_W * VLMAP_H * ck;
    }
    placed[(size_t)cls * msp + i] = make_float4(fx, fy, fz, p.w);
    cube[(size_t)cls * msp + i] = c;
}

// napp[e]: the points cube e receives; down[D_START + e]: the exclusive sum of old + received over the class's cubes; down[H_ADDED + cls]
__global__ __launch_bounds__(LM_ONE) void k_lmap_layout(int n_c, int n_s, int msp, const int* __restrict__ cube, const int* __restrict__ up, int* __restrict__ napp, int* __restrict__ down) {
    __shared__ int s_cnt[2 * LM_CUBES];
    __shared__ int s_w[LM_ONE / 64];
    const int t = threadIdx.x;
    for (int e = t; e < 2 * LM_CUBES; e += LM_ONE) s_cnt[e] = 0;
    __syncthreads();
    for (int g = t; g < n_c + n_s; g += LM_ONE) {
        const int cls = g >= n_c ? 1 : 0, c = cube[(size_t)cls * msp + (g - (cls ? n_c : 0))];
        if (c >= 0) atomicAdd(&s_cnt[cls * LM_CUBES + c], 1);                                      // a count: the order of the additions is not in it
    }
    __syncthreads();
    static_assert(LM_CUBES <= LM_ONE, "a cube per thread");
    for (int cls = 0; cls < 2; ++cls) {
        const int e = cls * LM_CUBES + t;
        const int app = t < LM_CUBES ? s_cnt[e] : 0, tot = t < LM_CUBES ? up[U_COUNT + e] + app : 0;
        int all_tot, all_app;
        const int ex = block_exclusive<LM_ONE / 64>(tot, s_w, all_tot);
        block_exclusive<LM_ONE / 64>(app, s_w, all_app);
        if (t < LM_CUBES) { napp[e] = app; down[D_START + e] = ex; }
        if (t == 0) down[H_ADDED + cls] = all_app;
    }
}

// cube x of class y in the new pool: its old points, then the received ones in stack order; down[D_COUNT + e] = their number
__global__ __launch_bounds__(LM_BLK) void k_lmap_append(int n_c, int n_s, int msp, int maxmap, const int* __restrict__ up, const int* __restrict__ napp, const float4* __restrict__ placed,
                                                        const int* __restrict__ cube, const float4* __restrict__ pool_old, float4* __restrict__ pool_new, int* __restrict__ down) {
    __shared__ int s_w[LM_WAVES];
    const int cls = blockIdx.y, c = blockIdx.x, e = cls * LM_CUBES + c, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int n_old = up[U_COUNT + e], app = napp[e], n_stack = cls ? n_s : n_c;
    if (t == 0) down[D_COUNT + e] = n_old + app;
    if (n_old + app == 0) return;
    const float4* src = pool_old + (size_t)cls * maxmap + up[U_START + e];
    float4* dst = pool_new + (size_t)cls * maxmap + down[D_START + e];                             // start + n_old + app <= old + received of the class <= maxmap (the host's capacity check)
    for (int i = t; i < n_old; i += LM_BLK) dst[i] = src[i];
    if (app == 0) return;
    const int* key = cube + (size_t)cls * msp;
    const float4* pts = placed + (size_t)cls * msp;
    int done = n_old;
    for (int i0 = 0; i0 < n_stack; i0 += LM_BLK) {
        const int i = i0 + t;
        const bool mine = i < n_stack && key[i] == c;
        const unsigned long long b = __ballot(mine);
        if (lane == 0) s_w[wave] = __popcll(b);
        __syncthreads();
        int before = 0, all = 0;
        for (int w = 0; w < LM_WAVES; ++w) { const int k = s_w[w]; before += w < wave ? k : 0; all += k; }
        if (mine) dst[done + before + __popcll(b & ((1ull << lane) - 1ull))] = pts[i];           // < n_old + app: k_lmap_layout counted the same keys
        done += all;
        __syncthreads();
    }
}

// step 7: filter A(leaf of the class, H) of valid cube x of class y, in place; down[D_COUNT + e] = the centroids
__global__ __launch_bounds__(LM_BLK) void k_lmap_refilter(int maxmap, const int* __restrict__ up, const int* __restrict__ napp, float inv_c, float inv_s, int H, int bits, float4* pool,
                                                          float4* tmp, int4* vox, int* sorted, int* evict, int* down) {
    __shared__ int s_hist[LM_WAVES][VCLOUD_MAX_HIST];
    __shared__ int s_brank[VCLOUD_MAX_HIST];
    __shared__ int s_w[LM_WAVES];
    const int cls = blockIdx.y, c = up[U_VALID + blockIdx.x], t = threadIdx.x, wave = t >> 6;
    if (c < 0) return;
    const int e = cls * LM_CUBES + c, n = up[U_COUNT + e] + napp[e];
    if (n == 0) return;                                                                            // k_lmap_append left the count 0
    const size_t base = (size_t)cls * maxmap + down[D_START + e];                                   // base + n <= (cls + 1) * maxmap, as in k_lmap_append
    float4* in = pool + base; float4* out = tmp + base;
    int4* vx = vox + base; int* so = sorted + base; int* ev = evict + base;
    const float inv = cls ? inv_s : inv_c;
    for (int i = t; i < n; i += LM_BLK) { vx[i] = voxel_of(in[i], inv, (unsigned)(H - 1)); ev[i] = 0; }
    for (int b = t; b < H; b += LM_BLK) for (int w = 0; w < LM_WAVES; ++w) s_hist[w][b] = 0;
    __syncthreads();
    // the stable counting sort by table entry: wave w owns the points [w * per, (w + 1) * per), per a multiple of 64
    const int per = ((n + LM_WAVES - 1) / LM_WAVES + 63) / 64 * 64, steps = per / 64;
    rank_piece<false>(wave * per, steps, n, vx, bits, nullptr, s_hist[wave]);
    int nv = 0, nonempty = 0;
    for (int b0 = 0; b0 < H; b0 += LM_BLK) {                                                        // histograms -> offsets, bucket-major, wave-minor; the rank of every bucket among the non-empty ones
        const int b = b0 + t;
        int cnt[LM_WAVES], tot = 0;
        for (int w = 0; w < LM_WAVES; ++w) { cnt[w] = b < H ? s_hist[w][b] : 0; tot += cnt[w]; }
        int all, all_f;
        int ex = nv + block_exclusive<LM_WAVES>(tot, s_w, all);
        const int exf = nonempty + block_exclusive<LM_WAVES>(tot > 0 ? 1 : 0, s_w, all_f);
        if (b < H) { for (int w = 0; w < LM_WAVES; ++w) { s_hist[w][b] = ex; ex += cnt[w]; } s_brank[b] = exf; }
        nv += all; nonempty += all_f;
    }
    __syncthreads();
    rank_piece<true>(wave * per, steps, n, vx, bits, so, s_hist[wave]);
    for (int p = t; p < nv; p += LM_BLK) if (p > 0) flag_eviction(p, vx, so, ev);
    __syncthreads();
    int n_evict = 0;
    for (int i0 = 0; i0 < n; i0 += LM_BLK) {                                                        // the exclusive sum of the flags in original index order
        const int i = i0 + t, v = i < n ? ev[i] : 0;
        int all;
        const int ex = n_evict + block_exclusive<LM_WAVES>(v, s_w, all);
        if (i < n) ev[i] = ex;
        n_evict += all;
    }
    __syncthreads();
    for (int p = t; p < nv; p += LM_BLK) emit_run(p, nv, n_evict, in, vx, so, ev, s_brank, out);    // positions < n_evict + nonempty <= n
    __syncthreads();
    const int n_out = n_evict + nonempty;
    for (int i = t; i < n_out; i += LM_BLK) in[i] = out[i];
    if (t == 0) down[D_COUNT + e] = n_out;
}

// step 8: cube x, corner then surf, behind the cubes before it; Rt: the host's R (9) and t (3) of the current pose
__global__ __launch_bounds__(LM_BLK) void k_lmap_publish(int maxmap, const int* __restrict__ down, const float4* __restrict__ pool, Mat34 Rt, float4* __restrict__ pub_world,
                                                         float4* __restrict__ pub_sensor) {
    __shared__ int s_w[LM_WAVES];
    const int c = blockIdx.x, t = threadIdx.x;
    int mine = 0;
    for (int k = t; k < c; k += LM_BLK) mine += down[D_COUNT + k] + down[D_COUNT + LM_CUBES + k];
    int off;
    block_exclusive<LM_WAVES>(mine, s_w, off);                                                      // off + this cube's points <= all points <= 2 * maxmap
    for (int cls = 0; cls < 2; ++cls) {
        const int e = cls * LM_CUBES + c, n = down[D_COUNT + e];
        const float4* src = pool + (size_t)cls * maxmap + down[D_START + e];
        for (int i = t; i < n; i += LM_BLK) {
            const float4 p = src[i];
            const double dx = (double)p.x - Rt.m[9], dy = (double)p.y - Rt.m[10], dz = (double)p.z - Rt.m[11];
            pub_world[off + i] = p;
            pub_sensor[off + i] = make_float4((float)((Rt.m[0] * dx + Rt.m[3] * dy) + Rt.m[6] * dz), (float)((Rt.m[1] * dx + Rt.m[4] * dy) + Rt.m[7] * dz),
                                              (float)((Rt.m[2] * dx + Rt.m[5] * dy) + Rt.m[8] * dz), p.w);
        }
        off += n;
    }
}

bool finite_all(const double* v, int n) { for (int k = 0; k < n; ++k) if (!std::isfinite(v[k])) return false; return true; }
int log2_of(int h) { int b = 0; while ((1 << b) < h) ++b; return b; }

// Eigen's quaternion product and quaternion * vector, [x y z w], in its order of operations
void quat_mul(const double* a, const double* b, double* o) {
    const double w = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
    const double x = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    const double y = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
    const double z = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
    o[0] = x; o[1] = y; o[2] = z; o[3] = w;
}
void quat_rot(const double* q, const double* v, double* o) {
    double uv[3] = {q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]};
    for (int k = 0; k < 3; ++k) uv[k] = uv[k] + uv[k];
    const double c[3] = {q[1] * uv[2] - q[2] * uv[1], q[2] * uv[0] - q[0] * uv[2], q[0] * uv[1] - q[1] * uv[0]};
    for (int k = 0; k < 3; ++k) o[k] = (v[k] + q[3] * uv[k]) + c[k];
}

struct Table { int start[2 * LM_CUBES]; int count[2 * LM_CUBES]; };

// one pass of a while loop of step 2 along `axis`: up = the contents move to the higher index and slot 0 is emptied
void shift_table(Table& T, const int axis, const bool up) {
    const int dim[3] = {VLMAP_W, VLMAP_H, VLMAP_D}, stride[3] = {1, VLMAP_W, VLMAP_W * VLMAP_H};
    const int a = axis, b = (axis + 1) % 3, c = (axis + 2) % 3;
    for (int cls = 0; cls < 2; ++cls)
        for (int u = 0; u < dim[b]; ++u)
            for (int v = 0; v < dim[c]; ++v) {
                const int base = cls * LM_CUBES + u * stride[b] + v * stride[c];
                if (up) for (int i = dim[a] - 1; i >= 1; --i) { T.start[base + i * stride[a]] = T.start[base + (i - 1) * stride[a]]; T.count[base + i * stride[a]] = T.count[base + (i - 1) * stride[a]]; }
                else for (int i = 0; i < dim[a] - 1; ++i) { T.start[base + i * stride[a]] = T.start[base + (i + 1) * stride[a]]; T.count[base + i * stride[a]] = T.count[base + (i + 1) * stride[a]]; }
                const int gone = base + (up ? 0 : dim[a] - 1) * stride[a];
                T.start[gone] = 0; T.count[gone] = 0;
            }
}

}  // namespace

struct __attribute__((visibility("hidden"))) vlmap_ctx : vilhost::Device {         // (its Fence members give it a destructor: not an exported one)  d_mem: up | down | napp | raw scans | stacks | placed | cube numbers | from-map | pools (2) | tmp | vox | sorted | evict | published (2)
    vlmap_config cfg;
    int msp = 0, maxmap = 0;
    vcloud_ctx* cloud = nullptr; vmap_ctx* reg = nullptr;                                           // private, through the public constructors
    char* h_io = nullptr; int* h_up = nullptr; int* h_down = nullptr;                               // pinned: points in either direction; what goes up; what comes down
    size_t o_up = 0, o_down = 0, o_napp = 0, o_raw = 0, o_stack = 0, o_placed = 0, o_cube = 0, o_fm = 0, o_pool[2] = {0, 0}, o_tmp = 0, o_vox = 0, o_sorted = 0, o_evict = 0, o_pub[2] = {0, 0};
    vilhost::Fence ready, done_c, done_s;                                                           // around the stacks' filters, which run on the vcloud_ctx's stream
    // the state of the header
    Table tab; int cur = 0;                                                                         // the table and the pool it points into
    int cen[3] = {5, 5, 3};
    double q_wmap_wodom[4] = {0, 0, 0, 1}, t_wmap_wodom[3] = {0, 0, 0}, q_last[4] = {0, 0, 0, 1}, t_last[3] = {0, 0, 0};
    int frame_count = 0, last_frame_count = 0; bool first_odom = true, broken = false;
    int n_map[2] = {0, 0}, n_pub = 0;
    int last_stack[2] = {0, 0}, last_fm[2] = {0, 0}; double last_M[12] = {}; bool has_M = false;      // what vlmap_debug_read reads
    vilhost::EventLog<VLMAP_NUM_KERNELS> prof;

    template <class T> T* at(size_t o) { return (T*)(d_mem + o); }
};

namespace {

void reset_state(vlmap_ctx* c) {
    memset(&c->tab, 0, sizeof c->tab);
    c->cen[0] = VLMAP_W / 2; c->cen[1] = VLMAP_H / 2; c->cen[2] = VLMAP_D / 2;
    for (int k = 0; k < 3; ++k) { c->q_wmap_wodom[k] = 0; c->t_wmap_wodom[k] = 0; c->q_last[k] = 0; c->t_last[k] = 0; }
    c->q_wmap_wodom[3] = 1; c->q_last[3] = 1;
    c->frame_count = 0; c->last_frame_count = 0; c->first_odom = true;
    c->n_map[0] = c->n_map[1] = 0; c->n_pub = 0;
    c->last_stack[0] = c->last_stack[1] = c->last_fm[0] = c->last_fm[1] = 0; c->has_M = false;
}

int read_points(vlmap_ctx* c, const void* d_src, const int n_have, float* out, const int32_t capacity, int32_t* n) {
    if (!n) return VIL_ERR_INVALID_ARGUMENT;
    *n = n_have;
    if (capacity < n_have || (n_have && !out)) return VIL_ERR_INVALID_ARGUMENT;
    if (n_have) {
        VILCHK(hipSetDevice(c->device));
        VILCHK(hipMemcpyAsync(c->h_io, d_src, 16 * (size_t)n_have, hipMemcpyDeviceToHost, c->stream));
        VILCHK(hipStreamSynchronize(c->stream));
        memcpy(out, c->h_io, 16 * (size_t)n_have);
    }
    return VIL_OK;
}

bool config_ok(const vlmap_config& g) {
    if (!vilcloud_stage::accepts(g.line_res, g.hist_size) || !vilcloud_stage::accepts(g.plane_res, g.hist_size)) return false;
    if (!(std::isfinite(g.cube_length) && g.cube_length > 0.0 && std::isfinite(g.cube_height) && g.cube_height > 0.0 && std::isfinite(g.publish_distance) && g.publish_distance >= 0.0)) return false;
    return g.max_scan_points >= 1 && g.max_map_points >= g.max_scan_points && g.max_map_points <= LM_MAX_POINTS;
}

}  // namespace

extern "C" {

void vlmap_default_config(vlmap_config* g) {
    if (!g) return;
    g->line_res = 0.2f; g->plane_res = 0.4f; g->hist_size = 512; g->publish_first_frame = 10; g->cube_length = 10.0; g->cube_height = 5.0; g->publish_distance = 2.0;
    g->publish_frames = 30; g->max_scan_points = 1 << 15; g->max_map_points = 1 << 19; g->reserved = 0;
}

int vlmap_create(int32_t device, const vlmap_config* cfg, vlmap_ctx** out) {
    vlmap_config g;
    vlmap_default_config(&g);
    if (cfg) g = *cfg;
    if (!out || !config_ok(g)) return VIL_ERR_INVALID_ARGUMENT;
    vlmap_ctx* c = new vlmap_ctx();
    c->cfg = g; c->msp = g.max_scan_points; c->maxmap = g.max_map_points;
    reset_state(c);
    const size_t N = (size_t)c->msp, M = (size_t)c->maxmap;
    vilhost::Arena a;
    c->o_up = a.take(4 * U_INTS);
    c->o_down = a.take(4 * D_INTS);
    c->o_napp = a.take(4 * 2 * LM_CUBES);
    c->o_raw = a.take(16 * 2 * N);
    c->o_stack = a.take(16 * 2 * N);
    c->o_placed = a.take(16 * 2 * N);
    c->o_cube = a.take(4 * 2 * N);
    c->o_fm = a.take(16 * 2 * M);
    c->o_pool[0] = a.take(16 * 2 * M);
    c->o_pool[1] = a.take(16 * 2 * M);
    c->o_tmp = a.take(16 * 2 * M);
    c->o_vox = a.take(16 * 2 * M);
    c->o_sorted = a.take(4 * 2 * M);
    c->o_evict = a.take(4 * 2 * M);
    c->o_pub[0] = a.take(16 * 2 * M);
    c->o_pub[1] = a.take(16 * 2 * M);
    hipError_t err = c->open(device, a.bytes);
    if (err == hipSuccess) err = c->pin(&c->h_io, 16 * 2 * M);
    if (err == hipSuccess) err = c->pin(&c->h_up, 4 * U_INTS);
    if (err == hipSuccess) err = c->pin(&c->h_down, 4 * D_INTS);
    if (err == hipSuccess) err = hipMemsetAsync(c->d_mem + c->o_down, 0, 4 * D_INTS, c->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(c->stream);
    int st = err == hipSuccess ? VIL_OK : VIL_ERR_DEVICE;
    if (st == VIL_OK) st = vcloud_create(device, c->msp, 1, &c->cloud);
    if (st == VIL_OK) st = vmap_create(device, &c->reg);
    if (st != VIL_OK) { vlmap_destroy(c); VILCHK(err); return st; }
    *out = c;
    return VIL_OK;
}

void vlmap_destroy(vlmap_ctx* c) {
    if (!c) return;
    vmap_destroy(c->reg); vcloud_destroy(c->cloud);
    c->close(c->prof);
    delete c;
}

int vlmap_reset(vlmap_ctx* c) {
    if (!c) return VIL_ERR_INVALID_ARGUMENT;
    reset_state(c);
    c->broken = false;
    return VIL_OK;
}

int vlmap_profile_enable(vlmap_ctx* c, int32_t enable) {
    if (!c) return VIL_ERR_INVALID_ARGUMENT;
    VILCHK(hipSetDevice(c->device));
    c->prof.on = enable != 0;
    return VIL_OK;
}
int vlmap_profile_read(vlmap_ctx* c, int64_t* launches6, double* total_ms6) {
    if (!c || !launches6 || !total_ms6) return VIL_ERR_INVALID_ARGUMENT;
    c->prof.read(launches6, total_ms6);
    return VIL_OK;
}

int vlmap_push_scan(vlmap_ctx* c, vil_ctx* solver, int32_t n_corner, const float* corner, int32_t n_surf, const float* surf, const double* q_wodom, const double* t_wodom,
                    const vil_options* opts, vlmap_summary* summary) {
    if (!c || !solver || !q_wodom || !t_wodom || n_corner < 0 || n_surf < 0 || n_corner > c->msp || n_surf > c->msp || (n_corner && !corner) || (n_surf && !surf)) return VIL_ERR_INVALID_ARGUMENT;
    if (!finite_all(q_wodom, 4) || !finite_all(t_wodom, 3)) return VIL_ERR_INVALID_ARGUMENT;
    const double qn2 = ((q_wodom[0] * q_wodom[0] + q_wodom[1] * q_wodom[1]) + q_wodom[2] * q_wodom[2]) + q_wodom[3] * q_wodom[3];
    if (!(qn2 > 0.0) || !std::isfinite(qn2)) return VIL_ERR_INVALID_ARGUMENT;
    if ((int64_t)c->n_map[0] + n_corner > c->maxmap || (int64_t)c->n_map[1] + n_surf > c->maxmap) return VIL_ERR_CAPACITY;
    if (c->broken) return VIL_ERR_DEVICE;
    c->prof.marks.clear();                                                                          // a call that failed after its first mark left them uncollected
    vil_options o;
    if (opts) o = *opts; else { vil_default_options(&o); o.max_iterations = 4; }
    const vlmap_config& g = c->cfg;
    const int n_in[2] = {n_corner, n_surf};

    vlmap_summary s;
    memset(&s, 0, sizeof s);
    // step 1
    double q[4], t[3], rt[3];
    quat_mul(c->q_wmap_wodom, q_wodom, q);
    quat_rot(c->q_wmap_wodom, t_wodom, rt);
    for (int k = 0; k < 3; ++k) t[k] = rt[k] + c->t_wmap_wodom[k];
    if (!finite_all(q, 4) || !finite_all(t, 3)) return VIL_ERR_INVALID_ARGUMENT;
    // step 2, on a copy of the table
    Table T = c->tab;
    int cen[3] = {c->cen[0], c->cen[1], c->cen[2]}, ctr[3];
    const int dim[3] = {VLMAP_W, VLMAP_H, VLMAP_D};
    for (int k = 0; k < 3; ++k) {
        ctr[k] = cube_of(t[k], k < 2 ? g.cube_length : g.cube_height, cen[k]);
        if (ctr[k] < -(1 << 16) || ctr[k] > (1 << 16)) return VIL_ERR_INVALID_ARGUMENT;          // further than any map reaches: nothing to keep, and the loops would not end soon
        while (ctr[k] < 3) { if (s.shift[k] < dim[k]) shift_table(T, k, true); ++ctr[k]; ++cen[k]; ++s.shift[k]; }
        while (ctr[k] >= dim[k] - 3) { if (s.shift[k] > -dim[k]) shift_table(T, k, false); --ctr[k]; --cen[k]; --s.shift[k]; }
    }
    // step 3: the valid cubes and where each starts in the from-map clouds
    int* up = c->h_up;
    memcpy(up + U_START, T.start, sizeof T.start); memcpy(up + U_COUNT, T.count, sizeof T.count);
    int nvalid = 0, fm[2] = {0, 0};
    for (int k = 0; k < 76; ++k) { up[U_VALID + k] = -1; up[U_FMOFF + k] = 0; up[U_FMOFF + 76 + k] = 0; }
    for (int i = ctr[0] - 2; i <= ctr[0] + 2; ++i)
        for (int j = ctr[1] - 2; j <= ctr[1] + 2; ++j)
            for (int k = ctr[2] - 1; k <= ctr[2] + 1; ++k)
                if (i >= 0 && i < VLMAP_W && j >= 0 && j < VLMAP_H && k >= 0 && k < VLMAP_D) {
                    const int e = i + VLMAP_W * j + VLMAP_W * VLMAP_H * k;
                    up[U_VALID + nvalid] = e;
                    for (int cls = 0; cls < 2; ++cls) { up[U_FMOFF + 76 * cls + nvalid] = fm[cls]; fm[cls] += T.count[cls * LM_CUBES + e]; }
                    ++nvalid;
                }
    s.n_corner_from_map = fm[0]; s.n_surf_from_map = fm[1];

    VILCHK(hipSetDevice(c->device));
    hipStream_t qs = c->stream;
    int* d_up = c->at<int>(c->o_up); int* d_down = c->at<int>(c->o_down); int* d_napp = c->at<int>(c->o_napp);
    float4* d_raw = c->at<float4>(c->o_raw); float4* d_stack = c->at<float4>(c->o_stack); float4* d_fm = c->at<float4>(c->o_fm);
    float4* pool_old = c->at<float4>(c->o_pool[c->cur]); float4* pool_new = c->at<float4>(c->o_pool[c->cur ^ 1]);
    const size_t N = (size_t)c->msp;
    VILCHK(hipMemcpyAsync(d_up, up, 4 * U_INTS, hipMemcpyHostToDevice, qs));
    for (int cls = 0; cls < 2; ++cls) {
        if (n_in[cls]) {
            memcpy(c->h_io + 16 * N * cls, cls ? surf : corner, 16 * (size_t)n_in[cls]);
            VILCHK(hipMemcpyAsync(d_raw + N * cls, c->h_io + 16 * N * cls, 16 * (size_t)n_in[cls], hipMemcpyHostToDevice, qs));
        }
        VILCHK(hipMemsetD32Async((hipDeviceptr_t)(d_down + H_RAW + cls), n_in[cls], 1, qs));
    }
    VILCHK(c->ready.record(qs));
    // step 4 on the cloud row's stream, step 3 on this one
    int st = vilcloud_stage::filter_resident(c->cloud, d_raw, d_down + H_RAW, n_corner, g.line_res, g.hist_size, d_stack, d_down + H_STACK, c->ready.ev, c->done_c);
    if (st == VIL_OK) st = vilcloud_stage::filter_resident(c->cloud, d_raw + N, d_down + H_RAW + 1, n_surf, g.plane_res, g.hist_size, d_stack + N, d_down + H_STACK + 1, c->ready.ev, c->done_s);
    if (st != VIL_OK) return st;
    VILCHK(hipSetDevice(c->device));
    VILCHK(c->prof.mark(K_GATHER, 1, qs));
    hipLaunchKernelGGL(k_lmap_gather, dim3(VLMAP_MAX_VALID, 2), dim3(LM_BLK), 0, qs, d_up, c->maxmap, pool_old, c->maxmap, d_fm);
    VILCHK(c->prof.mark(-1, 0, qs));
    VILCHK(hipStreamWaitEvent(qs, c->done_s.ev, 0));                                                  // (done_c precedes it on that stream)
    VILCHK(hipMemcpyAsync(c->h_down, d_down, 64, hipMemcpyDeviceToHost, qs));
    VILCHK(hipStreamSynchronize(qs));                                                               // host wait: the stacks' counts
    VILCHK(c->done_c.wait()); VILCHK(c->done_s.wait());
    VILCHK(hipGetLastError());
    const int n_cs = c->h_down[H_STACK], n_ss = c->h_down[H_STACK + 1];
    if (n_cs < 0 || n_cs > n_corner || n_ss < 0 || n_ss > n_surf) return VIL_ERR_DEVICE;
    s.n_corner_stack = n_cs; s.n_surf_stack = n_ss;
    c->last_stack[0] = n_cs; c->last_stack[1] = n_ss; c->last_fm[0] = fm[0]; c->last_fm[1] = fm[1]; c->has_M = false;
    // step 5
    st = vilmap_stage::set_map_resident(c->reg, fm[0], (const float*)d_fm, fm[1], (const float*)(d_fm + c->maxmap));
    if (st != VIL_OK) return st;
    const double* d_pose = nullptr;
    if (fm[0] > 10 && fm[1] > 50) {
        st = vilmap_stage::align_resident(c->reg, solver, n_cs, (const float*)d_stack, n_ss, (const float*)(d_stack + N), q, t, &o, &s.align);
        if (st != VIL_OK) return st;
        s.aligned = 1;
        d_pose = vilmap_stage::device_pose(c->reg);
    }
    double q_wm[4], t_wm[3];                                                                        // transformUpdate(), committed at the end
    {
        const double n2 = ((q_wodom[0] * q_wodom[0] + q_wodom[1] * q_wodom[1]) + q_wodom[2] * q_wodom[2]) + q_wodom[3] * q_wodom[3];
        const double inv[4] = {-q_wodom[0] / n2, -q_wodom[1] / n2, -q_wodom[2] / n2, q_wodom[3] / n2};
        quat_mul(q, inv, q_wm);
        quat_rot(q_wm, t_wodom, rt);
        for (int k = 0; k < 3; ++k) t_wm[k] = t[k] - rt[k];
    }
    // steps 6 and 7
    VILCHK(hipSetDevice(c->device));
    Mat34 Rt;
    double R[9];
    vilmap_stage::quat_to_R(q, R);
    for (int k = 0; k < 9; ++k) Rt.m[k] = R[k];
    for (int k = 0; k < 3; ++k) Rt.m[9 + k] = t[k];
    Geo geo; geo.cen[0] = cen[0]; geo.cen[1] = cen[1]; geo.cen[2] = cen[2]; geo.len = g.cube_length; geo.hgt = g.cube_height;
    float4* d_placed = c->at<float4>(c->o_placed); int* d_cube = c->at<int>(c->o_cube);
    const int n_st = n_cs + n_ss, blocks = (std::max(n_st, 1) + LM_BLK - 1) / LM_BLK;
    VILCHK(c->prof.mark(K_PLACE, 1, qs));
    hipLaunchKernelGGL(k_lmap_place, dim3(blocks), dim3(LM_BLK), 0, qs, n_cs, n_ss, c->msp, d_stack, Rt, d_pose, geo, d_placed, d_cube, (double*)(d_down + D_MATRIX));
    VILCHK(c->prof.mark(K_LAYOUT, 1, qs));
    hipLaunchKernelGGL(k_lmap_layout, dim3(1), dim3(LM_ONE), 0, qs, n_cs, n_ss, c->msp, d_cube, d_up, d_napp, d_down);
    VILCHK(c->prof.mark(K_APPEND, 1, qs));
    hipLaunchKernelGGL(k_lmap_append, dim3(LM_CUBES, 2), dim3(LM_BLK), 0, qs, n_cs, n_ss, c->msp, c->maxmap, d_up, d_napp, d_placed, d_cube, pool_old, pool_new, d_down);
    VILCHK(c->prof.mark(K_REFILTER, 1, qs));
    hipLaunchKernelGGL(k_lmap_refilter, dim3(VLMAP_MAX_VALID, 2), dim3(LM_BLK), 0, qs, c->maxmap, d_up, d_napp, 1.0f / g.line_res, 1.0f / g.plane_res, g.hist_size, log2_of(g.hist_size), pool_new,
                       c->at<float4>(c->o_tmp), c->at<int4>(c->o_vox), c->at<int>(c->o_sorted), c->at<int>(c->o_evict), d_down);
    // step 8: the decision needs the pose and the frame count only
    bool publish = false;
    if (c->first_odom) publish = c->frame_count >= g.publish_first_frame;
    else {
        const double d[3] = {c->t_last[0] - t[0], c->t_last[1] - t[1], c->t_last[2] - t[2]};
        double v[3];
        for (int k = 0; k < 3; ++k) v[k] = (R[k] * d[0] + R[3 + k] * d[1]) + R[6 + k] * d[2];
        publish = std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) > g.publish_distance || c->frame_count - c->last_frame_count > g.publish_frames;
    }
    if (publish) {
        VILCHK(c->prof.mark(K_PUBLISH, 1, qs));
        hipLaunchKernelGGL(k_lmap_publish, dim3(LM_CUBES), dim3(LM_BLK), 0, qs, c->maxmap, d_down, pool_new, Rt, c->at<float4>(c->o_pub[0]), c->at<float4>(c->o_pub[1]));
    }
    VILCHK(c->prof.mark(-1, 0, qs));
    VILCHK(hipMemcpyAsync(c->h_down, d_down, 4 * D_INTS, hipMemcpyDeviceToHost, qs));
    const hipError_t e_sync = hipStreamSynchronize(qs);                                             // host wait: the table
    if (e_sync != hipSuccess || hipGetLastError() != hipSuccess) { c->broken = publish; return VIL_ERR_DEVICE; }      // a failed publication may have overwritten the last one
    c->prof.collect();
    const int* dn = c->h_down;
    int tot[2] = {0, 0};
    for (int cls = 0; cls < 2; ++cls)
        for (int e = cls * LM_CUBES; e < (cls + 1) * LM_CUBES; ++e) {
            const int b = dn[D_START + e], k = dn[D_COUNT + e];
            if (b < 0 || k < 0 || (int64_t)b + k > c->maxmap) { c->broken = publish; return VIL_ERR_DEVICE; }
            tot[cls] += k;
        }
    if (dn[H_ADDED] < 0 || dn[H_ADDED] > n_cs || dn[H_ADDED + 1] < 0 || dn[H_ADDED + 1] > n_ss) { c->broken = publish; return VIL_ERR_DEVICE; }
    // commit
    memcpy(c->tab.start, dn + D_START, sizeof c->tab.start); memcpy(c->tab.count, dn + D_COUNT, sizeof c->tab.count);
    c->cur ^= 1;
    for (int k = 0; k < 3; ++k) c->cen[k] = cen[k];
    memcpy(c->last_M, dn + D_MATRIX, sizeof c->last_M); c->has_M = true;
    memcpy(c->q_wmap_wodom, q_wm, sizeof q_wm); memcpy(c->t_wmap_wodom, t_wm, sizeof t_wm);
    s.n_corner_added = dn[H_ADDED]; s.n_surf_added = dn[H_ADDED + 1]; s.n_corner_map = tot[0]; s.n_surf_map = tot[1];
    c->n_map[0] = tot[0]; c->n_map[1] = tot[1];
    if (c->first_odom) {
        memcpy(c->q_last, q, sizeof q); memcpy(c->t_last, t, sizeof t);
        c->last_frame_count = c->frame_count;
        if (publish) c->first_odom = false;
    } else if (publish) {
        memcpy(c->q_last, q, sizeof q); memcpy(c->t_last, t, sizeof t);
        c->last_frame_count = c->frame_count;
    }
    if (publish) {
        c->n_pub = tot[0] + tot[1];
        memset(c->tab.count, 0, sizeof c->tab.count);
        c->n_map[0] = c->n_map[1] = 0;
        c->q_wmap_wodom[0] = c->q_wmap_wodom[1] = c->q_wmap_wodom[2] = 0; c->q_wmap_wodom[3] = 1;
        c->t_wmap_wodom[0] = c->t_wmap_wodom[1] = c->t_wmap_wodom[2] = 0;
    }
    ++c->frame_count;
    memcpy(s.q_w_curr, q, sizeof q); memcpy(s.t_w_curr, t, sizeof t);
    s.published = publish ? 1 : 0; s.frame_count = c->frame_count;
    if (summary) *summary = s;
    return VIL_OK;
}

int vlmap_read_published(vlmap_ctx* c, int32_t frame, float* out_xyzi, int32_t capacity, int32_t* n) {
    if (!c || (frame != VLMAP_FRAME_WORLD && frame != VLMAP_FRAME_SENSOR)) return VIL_ERR_INVALID_ARGUMENT;
    return read_points(c, c->d_mem + c->o_pub[frame], c->n_pub, out_xyzi, capacity, n);
}

int vlmap_read_cube(vlmap_ctx* c, int32_t cls, int32_t index, float* out_xyzi, int32_t capacity, int32_t* n) {
    if (!c || cls < 0 || cls > 1 || index < 0 || index >= LM_CUBES) return VIL_ERR_INVALID_ARGUMENT;
    const int e = cls * LM_CUBES + index;
    return read_points(c, c->at<float4>(c->o_pool[c->cur]) + (size_t)cls * c->maxmap + c->tab.start[e], c->tab.count[e], out_xyzi, capacity, n);
}

int vlmap_debug_write_cube(vlmap_ctx* c, int32_t cls, int32_t index, int32_t n, const float* xyzi) {
    if (!c || cls < 0 || cls > 1 || index < 0 || index >= LM_CUBES || n < 0 || (n && !xyzi)) return VIL_ERR_INVALID_ARGUMENT;
    const int e = cls * LM_CUBES + index;
    int64_t end = 0;                                                                                // behind every other cube of the class
    for (int k = cls * LM_CUBES; k < (cls + 1) * LM_CUBES; ++k) if (k != e && c->tab.count[k]) end = std::max<int64_t>(end, (int64_t)c->tab.start[k] + c->tab.count[k]);
    if (end + n > c->maxmap || (int64_t)c->n_map[cls] - c->tab.count[e] + n > c->maxmap) return VIL_ERR_CAPACITY;
    if (n) {
        VILCHK(hipSetDevice(c->device));
        memcpy(c->h_io, xyzi, 16 * (size_t)n);
        VILCHK(hipMemcpyAsync(c->at<float4>(c->o_pool[c->cur]) + (size_t)cls * c->maxmap + end, c->h_io, 16 * (size_t)n, hipMemcpyHostToDevice, c->stream));
        VILCHK(hipStreamSynchronize(c->stream));
    }
    c->n_map[cls] += n - c->tab.count[e];
    c->tab.start[e] = (int)end; c->tab.count[e] = n;
    return VIL_OK;
}

int vlmap_debug_read(vlmap_ctx* c, int32_t stage, float* out_xyzi, int32_t capacity, int32_t* n) {
    if (!c) return VIL_ERR_INVALID_ARGUMENT;
    if (stage == VLMAP_DBG_CORNER_STACK || stage == VLMAP_DBG_SURF_STACK) {
        const int cls = stage - VLMAP_DBG_CORNER_STACK;
        return read_points(c, c->at<float4>(c->o_stack) + (size_t)cls * c->msp, c->last_stack[cls], out_xyzi, capacity, n);
    }
    if (stage == VLMAP_DBG_CORNER_FROM_MAP || stage == VLMAP_DBG_SURF_FROM_MAP) {
        const int cls = stage - VLMAP_DBG_CORNER_FROM_MAP;
        return read_points(c, c->at<float4>(c->o_fm) + (size_t)cls * c->maxmap, c->last_fm[cls], out_xyzi, capacity, n);
    }
    if (stage == VLMAP_DBG_MATRIX) {
        if (!n) return VIL_ERR_INVALID_ARGUMENT;
        *n = c->has_M ? 6 : 0;
        if (capacity < *n || (*n && !out_xyzi)) return VIL_ERR_INVALID_ARGUMENT;
        if (*n) memcpy(out_xyzi, c->last_M, sizeof c->last_M);
        return VIL_OK;
    }
    return VIL_ERR_INVALID_ARGUMENT;
}

}  // extern "C"
