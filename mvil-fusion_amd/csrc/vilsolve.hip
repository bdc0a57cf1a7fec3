// libvilsolve.so -- C-ABI (include/vilsolve.h; its lab bench: include/vilsolve_debug.h) over the gfx950 kernels.
// Replaces, for mVIL-Fusion's Estimator::optimization() (estimator.cpp:1124-1687), the ceres::Problem
// construction + ceres::Solve + MarginalizationInfo machinery.  No CPU fallback: every compute entry
// point needs a HIP device and returns VIL_ERR_DEVICE otherwise.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include <mutex>
#include <thread>
#include <array>
#include <map>

#include "../../include/vilsolve_debug.h"
#include "../../include/vilsolve_debug_ww.h"
#include "vil_internal.h"
#include "vil_comm.hpp"
#include "vil_resident.hpp"
#include "vil_tuning.hpp"
#include "vil_coop.hpp"
#include "vil_dev.hpp"
#include "vil_finish.hpp"
#include "vil_sweep.hpp"
#include "vil_eval.hpp"
#include "vil_step.hpp"
#include "vil_iter.hpp"
#include "vil_marg.hpp"
#include "vil_window.hpp"

// vilpersist.hip: the persistent solve kernel k_solve<2 | 5> (compiled in its own translation unit: vil_math.hpp, VIL_OPAQUE_TID)
const void* vil_k_solve_fn(int vis_ts);
void vil_k_solve_launch(int vis_ts, unsigned grid, size_t lds, hipStream_t stream, const DevP& P, const SolveOpts& O, long long budget_ticks);

namespace {

// One device allocation per uploaded window: [tables | work space].  The tables (everything the caller hands over) are
// assembled in a PINNED host image and go up in one DMA; the work space (partial records, systems, step vectors) exists on the
// device only and is cleared by a memset -- it used to travel as zeros through a pageable staging vector.
struct Arena {
    vilhost::Grown<char, true> h; size_t hsize = 0;    // pinned host image of the tables
    vilhost::Grown<char> d;                            // device
    size_t ssize = 0;                                  // work-space bytes
    bool grow(size_t need) {
        if (need <= h.cap) return true;
        size_t ncap = h.cap ? h.cap : (size_t)1 << 20;
        while (ncap < need) ncap *= 2;
        vilhost::Grown<char, true> nh;                 // (reserve() keeps no contents: the image moves into a new block, the old one goes with nh)
        if (nh.reserve(ncap, ncap) != hipSuccess) return false;
        if (hsize) memcpy(nh.p, h.p, hsize);
        h = std::move(nh);
        return true;
    }
    // returns (size_t)-1 when the pinned image cannot grow
    size_t take(size_t bytes) { const size_t o = (hsize + 255) & ~size_t(255); if (!grow(o + bytes)) return (size_t)-1; if (o > hsize) memset(h.p + hsize, 0, o - hsize); hsize = o + bytes; return o; }
    size_t take_scratch(size_t bytes) { const size_t o = (ssize + 255) & ~size_t(255); ssize = o + bytes; return o; }
    void reset() { hsize = 0; ssize = 0; }
};

}  // namespace

#define VIL_MAX_CHUNK 24       // iterations enqueued without a host round trip (the first solve of an upload: vil_solve_resident); vil_profile_enable sizes its events for it
#define VIL_CHC_MAX 16384      // entries of the chain workgroup's gather table (K = 20: ~7000)
#define VIL_SFLAG_MAX 4096      // sweep workgroups a one-launch iteration may have (configs[2]: ~600)
// The launch structure of an uploaded window, decided once per upload (choose_structure): every launch of a solve and the solve's ladder read it
struct Structure {
    int chain = 0, chain_rs = 0, prechain = 0, rs_merged = 0, n_ww = 0, n_gather = 0, n_sw = 0;      // what DevP carries of it (vil_dev.hpp)
    bool fused = false, persist = false;          // one launch per iteration (k_iter) / the whole solve in one resident launch (k_solve)
    const void* sweep_fn = nullptr; const void* step_fn = nullptr; const void* iter_fn = nullptr;      // k_sweep<2 | 5>, the k_step variant, k_iter<2 | 5>: granted and launched
    size_t lds_sweep = 0, lds_step = 0, lds_iter = 0, lds_solve = 0;
    int n_sweep = 0, n_reduce = 0, n_reduce_po = 0, n_gather_m = 0, cap_fused = -1;       // workgroups: sweep roles, k_reduce (all / pose-only gather), gather of the merged launch; cap_fused: of k_iter, at lds_iter, the device holds at once (vil_solve_batch)
};
struct vil_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    Comm comm;                     // multi-GPU: rank, world, the transport and the owner table of the per-iteration message (vil_comm.hpp)
    Arena ar;
    vilhost::Fence dep_ev;                                 // orders the solve after a producer stream (vil_solve_device_lidar: its handle, in a hipStreamWaitEvent)
    vilhost::Fence up_sent;                                // the DMA out of the pinned image must finish before the image is rewritten
    DevP P;                        // device pointers
    bool uploaded = false;
    int resident_kind = 0;         // 1: a window handed over through vil_upload / vil_solve (the only kind vil_solve_resident accepts);
                                   // 2: a derived problem of vil_marginalize / vil_eval_factors / vil_linearize (they replace the resident window)
    void invalidate() { uploaded = false; resident_kind = 0; }      // nothing is resident: the next solve needs an upload
    int K = 0, L = 0, D = 0, NS = 0;
    size_t off_x0 = 0;             // backup of the uploaded state (device)
    double* d_x0 = nullptr;
    double* d_xsave = nullptr;        // the state the solve at hand started from (written by its init launch)
    int drop_role = -1, drop_launch = -1;      // vil_debug_drop_flag: armed for the next solve
    bool in_batch = false;         // this solve is one of a vil_solve_batch (shared gate, no persistent solve)
    int rung_fail_run[2] = {0, 0}, rung_cooldown[2] = {0, 0};      // launch-structure ladder (vil_solve_resident): consecutive give-ups of the persistent solve / the one-launch iteration, solves they sit out
    int64_t n_recovered = 0, n_aborted = 0;    // solves whose one-launch attempt gave up and were re-run with two launches per iteration / that failed on both
    bool reset_pending = false;       // vil_reset_state called, the copy not launched yet
    std::vector<int> plane_perm, edge_perm;   // sorted index -> caller index
    Structure ls;                  // the launch structure of the uploaded window (choose_structure)
    std::map<const void*, int> lds_granted;      // per kernel: the largest dynamic-LDS size granted so far (grant_lds)
    std::map<const void*, std::pair<size_t, int>> coop_caps;      // per kernel: (dynamic-LDS size probed last, workgroups the device holds at once AT that size) -- coop_capacity
    int vis_gm = 0;                      // doubles of operand rows the largest visual chunk of the uploaded window needs (vil_sweep.hpp)
    size_t span = 0;               // doubles of one linear-system set (SysBuf::ar): the multi-GPU all-reduce message
    vilhost::Grown<int> d_status;
    vilhost::Grown<Ctl, true> h_ctl;          // pinned
    vilhost::Grown<int, true> h_word;         // pinned: status words read back from the device (16 of them)
    vilhost::Mapped h_mirror; Ctl* d_hctl = nullptr; int* d_hseq = nullptr; double* d_hstate = nullptr; size_t mirror_ns = 0;      // pinned + mapped: Ctl | sequence word | final state, written by solve_finish (vil_finish.hpp)
    bool no_poll = false;          // VIL_NO_POLL=1: copy + synchronise instead of polling the mirror
    bool mirror_state = false;     // the mirror holds the final state of the last solve (vil_download_state needs no device operation)
    vilhost::Grown<double, true> h_pin;       // pinned scratch
    vilhost::Grown<char> marg_ws;             // device work space of vil_marginalize
    unsigned long long* d_marg_ts = nullptr;      // phase stamps of the last marginalisation's kernels (vil_debug_marg_stamps): a place in marg_ws
    std::vector<int> prior_joff;
    bool sharded = false;          // the resident problem is this rank's shard of the factor set
    // hipGraph of a chunk of iterations, reused by repeated solves of one upload (key: chunk length, options)
    struct ChunkGraph { int n; SolveOpts so; hipGraphExec_t exec; };
    std::vector<ChunkGraph> graphs;
    int use_graph = -1;            // VIL_GRAPH=0 disables (tuning build)
    vilhost::Grown<int> d_imu_perm;      // (vil_sweep.hpp, sweep_imu: entry order of the IMU roles)
    // (a few tables by key: a tracker alternates between the prior structures of its two marginalisation kinds, and a rebuild -- entries, sort, copy -- is ~80 us of host time)
    struct ChTab { std::vector<int> key; FrameStage st; int n = 0; unsigned long long used = 0; const int* d() const { return (const int*)st.d.p; } };      // (the table travels like a pushed frame)
    ChTab chtabs[4]; int chtab_cur = 0; unsigned long long chtab_clock = 0;      // gather table of the chain workgroup (vil_prechain.hpp)
    bool graph_failed = false;     // a chunk could not be captured / instantiated: direct launches from then on
    int fail_capture = 0;          // vil_debug_fail_graph_capture: that many captures are treated as failed
    int solve_gen = 0;             // generation counter of the helper-workgroup flags (Ctl::gen)
    int solves_since_upload = 0;
    bool split = false;            // sweep + gather fill set 0, the collective sums it into set 1, the step kernel reads set 1
    bool force_split = false;      // vil_debug_set_split: that plumbing on a single rank
    int launch_mode = 0;           // vil_debug_set_launch_mode: 0 = the library's choice, 1 = no merged launch, 2 = no chain workgroup, 3 = sweep + merged gather / step launch (no one-launch iteration)
    int last_live = 5;             // live sweep launches of the previous solve (sizes the first launch chunk)
    int recent_live[8] = {5, 5, 5, 5, 5, 5, 5, 5}; int recent_at = 0;      // ... of the last eight solves: the first solve of an upload (a tracker's image) is sized by their maximum
    // ---- window residency across frames (vil_lidar_*, vil_set_gauge_fix, vil_marginalize_resident) --------------------------------
    LidarSlabs lidar;              // LiDAR frame slabs (vil_resident.hpp)
    bool lidar_resident = false;   // the resident problem takes its point factors from the slabs
    bool gauge_on = false;
    struct MargMeta {              // what vil_marginalize_resident needs to know about the resident window (captured at upload)
        std::vector<int> prior_kind, prior_index; bool has_prior = false;
        std::vector<char> obs0;    // frames observing a landmark anchored in frame 0
        int n_lm0 = 0; bool imu01 = false; bool lidar0 = false; bool use_td = false;
        std::vector<int> icp_ids, lps_ids;
    } mm;
    Window win;                    // the fully resident window (vil_win_*: vil_resident.hpp, vil_window.hpp)
    bool profiling = false, stamps = false; long long period_n = 0;
    std::vector<unsigned long long> last_stamps;      // raw stamps of the last profiled solve (vil_debug_read_stamps)
    int wg_launch = -1;      // (vil_profile_workgroups)
    vilhost::Grown<long long> d_prof; double phase_us[VIL_PROF_SLOTS] = {0}; long long phase_n = 0;      // phase stamps of the one-launch iterations (vil_profile_phases)
    std::vector<hipEvent_t> ev, ev_mid, ev_coll;
    vil_profile prof = {0, 0.0, 0, 0.0, 0.0};
    // what only the context can release (vil_destroy has selected the device and drained the stream); every member above then frees itself, with the
    // device still current and the stream gone (vil_host.hpp)
    ~vil_ctx() {
        for (auto& e : ev) hipEventDestroy(e);
        for (auto& e : ev_mid) hipEventDestroy(e);
        for (auto& e : ev_coll) hipEventDestroy(e);
        for (auto& g : graphs) hipGraphExecDestroy(g.exec);
        comm.release(device);
        if (stream) hipStreamDestroy(stream);
    }
};

// pinned, device-mapped mirror [Ctl | sequence word (64 B) | final state (ns doubles)]; grow-only
static int ensure_mirror(vil_ctx* c, size_t ns) {
    if (c->h_mirror.h && ns <= c->mirror_ns) return VIL_OK;
    if (c->stream) HIPCHK(hipStreamSynchronize(c->stream));       // nobody is writing the old one
    c->d_hctl = nullptr; c->d_hseq = nullptr; c->d_hstate = nullptr; c->mirror_ns = 0; c->mirror_state = false;
    const size_t cap = ns + ns / 2 + 256, bytes = sizeof(Ctl) + 64 + 8 * cap;
    HIPCHK(c->h_mirror.open(bytes));                              // (releases the old one first)
    void* const dp = c->h_mirror.d;
    c->d_hctl = (Ctl*)dp; c->d_hseq = (int*)((char*)dp + sizeof(Ctl)); c->d_hstate = (double*)((char*)dp + sizeof(Ctl) + 64);
    c->mirror_ns = cap;
    return VIL_OK;
}

// static LDS of a kernel as the loaded code object reports it (StepShared is only part of what k_step carries: the gather and tile roles keep scratch arrays there)
static size_t step_static_lds(const void* fn) {
    // (a property of the code object: asked once per kernel and process -- hipFuncGetAttributes is a few microseconds of driver time, and every upload, i.e. every
    //  image of a tracker, asked five times)
    static std::mutex mu; static std::vector<std::pair<const void*, size_t>> known;
    std::lock_guard<std::mutex> lk(mu);
    for (const auto& e : known) if (e.first == fn) return e.second;
    hipFuncAttributes fa;
    if (hipFuncGetAttributes(&fa, fn) != hipSuccess) { (void)hipGetLastError(); return (size_t)64 * 1024; }
    known.emplace_back(fn, (size_t)fa.sharedSizeBytes);
    return (size_t)fa.sharedSizeBytes;
}
// hipFuncSetAttribute is not free: a kernel's dynamic-LDS limit is raised only when it needs more than it was granted before
static hipError_t grant_lds(vil_ctx* c, const void* fn, size_t bytes) {
    int& granted = c->lds_granted[fn];
    const hipError_t e = (int)bytes > granted ? hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) : hipSuccess;
    if (e == hipSuccess) granted = std::max(granted, (int)bytes);
    return e;
}
// workgroups of a kernel the device holds at once AT THAT dynamic-LDS size (vil_coop.hpp): probed again when the size changes (42 kB at K = 10: 3 per CU, 95 kB at K = 20: 1)
static int coop_capacity(vil_ctx* c, const void* fn, size_t lds) {
    auto it = c->coop_caps.find(fn);
    if (it == c->coop_caps.end() || it->second.first != lds) it = c->coop_caps.insert_or_assign(fn, std::make_pair(lds, vilcoop::capacity(fn, VIL_STEP_THREADS, lds, c->device))).first;
    return it->second.second;
}
static SolveOpts to_dev_opts(const vil_options* o) {
    SolveOpts s;
    memset(&s, 0, sizeof s);            // compared bytewise as the key of the cached iteration graphs
    s.max_iterations = o->max_iterations; s.jacobi_scaling = o->jacobi_scaling;
    s.visual_loss = o->visual_loss; s.lidar_loss = o->lidar_loss; s.rel_loss = o->rel_loss; s.autodiff_quirk = o->autodiff_quirk;
    s.precision = o->precision == 1 ? 1 : 0;
    s.function_tolerance = o->function_tolerance; s.gradient_tolerance = o->gradient_tolerance; s.parameter_tolerance = o->parameter_tolerance;
    s.max_radius = o->max_radius; s.min_relative_decrease = o->min_relative_decrease; s.min_mu = o->min_mu; s.max_mu = o->max_mu;
    s.visual_loss_scale = o->visual_loss_scale; s.lidar_loss_scale = o->lidar_loss_scale; s.rel_loss_scale = o->rel_loss_scale;
    return s;
}

static void quat_to_R_host(const double* q, double* R) {
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - w * z); R[2] = 2 * (x * z + w * y);
    R[3] = 2 * (x * y + w * z); R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - w * x);
    R[6] = 2 * (x * z - w * y); R[7] = 2 * (y * z + w * x); R[8] = 1 - 2 * (x * x + y * y);
}

// test hook (vil_debug_dense_solve): the step's dense factorisation + back substitution on a matrix of the caller's -- one workgroup, the tiled LDS layout of vil_step.hpp.
// RW: what the one-launch iteration runs (chol_dense / back_subst_cols); otherwise the look-ahead factorisation and the back substitution with inverted diagonal tiles.
// WWS (vil_debug_dense_solve_ww): the matrix is A - S WW S, subtracted the way the step subtracts the chain's W W^T -- on the factorisation's register tiles, out of
// chWW in the lane-major tile layout (k_debug_ww_fill wrote it through ww_idx), with the scales sc (rhs row: its column's scale only).
__global__ void k_debug_ww_fill(const double* WW /* (D+1) x (D+1) row major, every entry as it stands */, double* chWW, int D, double pad /* tile elements past row / column D */) {
    const int R = D + 1, T = (R + 15) >> 4, n = ((T * (T + 1)) >> 1) << 8;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += gridDim.x * blockDim.x) {
        const int g = e >> 8, r = (e >> 4) & 15, c = e & 15;
        int I = 0; while ((I + 1) * (I + 2) / 2 <= g) ++I;
        const int J = g - I * (I + 1) / 2, i = (I << 4) + r, j = (J << 4) + c;
        chWW[vd::ww_idx(g, r, c)] = (i < R && j < R) ? WW[(size_t)i * R + j] : pad;
    }
}
template <int SLOTS, bool RW, bool WWS = false>
__global__ __launch_bounds__(VIL_STEP_THREADS) void k_debug_dense(const double* Ain /* (D+1) x (D+1) row major: lower triangle, last row = right-hand side */, double* Lout, double* xout, int* okout, int D, const double* chWW = nullptr, const double* scin = nullptr) {
    extern __shared__ double dbgA[];
    __shared__ vd::StepShared s;
    const int t = threadIdx.x, R = D + 1, T = (R + 15) >> 4, NTL = ((T * (T + 1)) >> 1) * TILE_SZ;
    if (t == 0) { int g = 0; for (int I = 0; I < T; ++I) for (int J = 0; J <= I; ++J) { s.tI[g] = (unsigned char)I; s.tJ[g] = (unsigned char)J; ++g; } }
    for (int e = t; e < NTL; e += blockDim.x) dbgA[e] = 0.0;
    if constexpr (WWS) { for (int e = t; e < D; e += blockDim.x) s.sc[e] = scin[e]; }
    __syncthreads();
    for (int e = t; e < R * R; e += blockDim.x) { const int i = e / R, j = e - i * R; if (j <= i && j < D) dbgA[vd::tl_idx(i, j)] = Ain[e]; }
    __syncthreads();
    bool ok;
    if constexpr (WWS) {
        auto pre = [&](vd::d4* Creg, const int* tIJ) {
            double ww[SLOTS][4];
            vd::ww_tiles_load<SLOTS>(chWW, tIJ, t & 63, ww);
            vd::ww_tiles_sub<SLOTS>(Creg, tIJ, t & 63, ww, s.sc, D);
        };
        if constexpr (RW) ok = vd::chol_dense<SLOTS>(dbgA, D, s, pre); else ok = vd::chol_lookahead<SLOTS, false>(dbgA, D, s, pre);
    } else
    if constexpr (RW) ok = vd::chol_dense<SLOTS>(dbgA, D, s); else ok = vd::chol_lookahead<SLOTS, false>(dbgA, D, s);
    __syncthreads();
    for (int e = t; e < R * R; e += blockDim.x) { const int i = e / R, j = e - i * R; Lout[e] = (j < i && j < D) ? dbgA[vd::tl_idx(i, j)] : ((j == i && i < D) ? 1.0 / s.dinv[i] : 0.0); }
    __syncthreads();
    if (ok) { if constexpr (RW) vd::back_subst_cols(dbgA, D, s); else vd::back_subst(dbgA, D, s); }
    __syncthreads();
    for (int e = t; e < D; e += blockDim.x) xout[e] = ok ? s.y[e] : 0.0;
    if (t == 0) okout[0] = ok ? 1 : 0;
}
extern "C" {

int vil_abi_version(void) { return VIL_ABI_VERSION; }

const char* vil_strerror(int st) {
    switch (st) {
        case VIL_OK: return "ok";
        case VIL_ERR_INVALID_ARGUMENT: return "invalid argument";
        case VIL_ERR_DEVICE: return "HIP device error (no device / runtime failure)";
        case VIL_ERR_NON_FINITE: return "non-finite cost or state";
        case VIL_ERR_NOT_POSITIVE_DEFINITE: return "reduced system not positive definite";
        case VIL_ERR_COMM: return "RCCL error";
        case VIL_ERR_UNSUPPORTED: return "unsupported configuration";
        case VIL_ERR_CAPACITY: return "capacity exceeded";
    }
    return "unknown";
}

int vil_reduced_dim(int K) { return 15 * K + 7; }
void vil_prior_capacity(int K, int* n_max, int* nblk_max, int* x0_max) {
    if (n_max) *n_max = 6 * K + 16;
    if (nblk_max) *nblk_max = K + 4;
    if (x0_max) *x0_max = 7 * K + 9 + 7 + 1 + 16;
}
void vil_default_options(vil_options* o) {
    o->max_iterations = 30; o->max_time_s = 0.05;
    o->function_tolerance = 1e-6; o->gradient_tolerance = 1e-10; o->parameter_tolerance = 1e-8;
    o->initial_radius = 1e4; o->max_radius = 1e16; o->min_relative_decrease = 1e-3;
    o->min_mu = 1e-8; o->max_mu = 1.0; o->jacobi_scaling = 1;
    o->visual_loss = VIL_LOSS_CAUCHY; o->visual_loss_scale = 1.0;
    o->lidar_loss = VIL_LOSS_HUBER; o->lidar_loss_scale = 0.1;
    o->rel_loss = VIL_LOSS_CAUCHY; o->rel_loss_scale = 1.0;
    o->autodiff_quirk = 1; o->precision = 0;
}

static int ctx_open(vil_ctx* c) {
    HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    HIPCHK(c->d_status.reserve(1, 1));
    HIPCHK(hipMemset(c->d_status.p, 0, sizeof(int)));
    HIPCHK(c->h_ctl.reserve(1, 1));
    HIPCHK(c->h_word.reserve(16, 16));      // small status reads land in PINNED memory (an asynchronous copy into pageable memory goes through the runtime's staging path)
    return VIL_OK;
}
int vil_create(const vil_device_cfg* cfg, vil_ctx** out) {
    if (!cfg || !out) return VIL_ERR_INVALID_ARGUMENT;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { fprintf(stderr, "[vilsolve] no HIP device: the hot path has no CPU fallback\n"); return VIL_ERR_DEVICE; }
    if (cfg->device < 0 || cfg->device >= ndev) return VIL_ERR_INVALID_ARGUMENT;
    HIPCHK(hipSetDevice(cfg->device));
    vil_ctx* c = new vil_ctx();
    c->device = cfg->device; c->comm.rank = cfg->rank; c->comm.world = cfg->world > 0 ? cfg->world : 1;
    c->no_poll = getenv("VIL_NO_POLL") != nullptr;
    memset(&c->P, 0, sizeof c->P);
    const int st = ctx_open(c);
    if (st != VIL_OK) vil_destroy(c); else *out = c;      // (a context that could not be opened goes the way every context goes)
    return st;
}

void vil_destroy(vil_ctx* c) {
    if (!c) return;
    hipSetDevice(c->device);
    if (c->stream) hipStreamSynchronize(c->stream);
    delete c;
}

static int validate(const vil_problem* p, const vil_state* s, bool device_lidar = false, bool win = false) {
    if (!p || !s) return VIL_ERR_INVALID_ARGUMENT;
    if (p->K < 1 || p->L < 0 || s->K != p->K || s->L != p->L) return VIL_ERR_INVALID_ARGUMENT;
    if (!s->pose || !s->speedbias || !s->ex_pose || !s->td || (p->L > 0 && !s->inv_depth)) return VIL_ERR_INVALID_ARGUMENT;
    if (15 * p->K + 7 > 320) return VIL_ERR_UNSUPPORTED;   // K <= 20 (step kernel work space)
    const bool res_lidar = p->n_plane == VIL_LIDAR_RESIDENT && p->n_edge == VIL_LIDAR_RESIDENT;
    if (res_lidar) device_lidar = true;          // the tables are the context's slabs: nothing of the caller's to check
    if (p->n_vis < 0 || p->n_imu < 0 || p->n_icp < 0 || p->n_lps < 0 || (!res_lidar && (p->n_plane < 0 || p->n_edge < 0)) || p->prior.n < 0) return VIL_ERR_INVALID_ARGUMENT;
    if (p->n_icp + p->n_lps > 12) return VIL_ERR_UNSUPPORTED;   // reference trims to 5 + 7 (estimator.cpp:1283-1286,1345-1348)
    if (p->prior.n > 512 || p->prior.nblk > 256) return VIL_ERR_UNSUPPORTED;
    // a table may be NULL only when its count is zero
    if (p->n_vis > 0 && (!p->vis_i || !p->vis_j || !p->vis_l || !p->vis_const)) return VIL_ERR_INVALID_ARGUMENT;
    if (p->n_imu > 0 && (!p->imu_i || !p->imu_j || (!p->imu_const && !win))) return VIL_ERR_INVALID_ARGUMENT;
    if (p->n_icp > 0 && (!p->icp_ids || !p->icp_const)) return VIL_ERR_INVALID_ARGUMENT;
    if (p->n_lps > 0 && (!p->lps_ids || !p->lps_const)) return VIL_ERR_INVALID_ARGUMENT;
    if (!device_lidar && p->n_plane > 0 && (!p->plane_pose || !p->plane_const)) return VIL_ERR_INVALID_ARGUMENT;
    if (!device_lidar && p->n_edge > 0 && (!p->edge_pose || !p->edge_const)) return VIL_ERR_INVALID_ARGUMENT;
    for (int f = 0; f < p->n_vis; ++f) {
        if (p->vis_l[f] < 0 || p->vis_l[f] >= p->L || p->vis_i[f] < 0 || p->vis_i[f] >= p->K || p->vis_j[f] < 0 || p->vis_j[f] >= p->K) return VIL_ERR_INVALID_ARGUMENT;
        if (p->vis_i[f] == p->vis_j[f]) return VIL_ERR_INVALID_ARGUMENT;     // the reference never builds such a factor (estimator.cpp:1205: `if (imu_i == imu_j) continue;`)
        if (f && p->vis_l[f] < p->vis_l[f - 1]) return VIL_ERR_INVALID_ARGUMENT;
        if (f && p->vis_l[f] == p->vis_l[f - 1] && p->vis_i[f] != p->vis_i[f - 1]) return VIL_ERR_INVALID_ARGUMENT;
    }
    if (!device_lidar) {
        for (int f = 0; f < p->n_plane; ++f) if (p->plane_pose[f] < 0 || p->plane_pose[f] >= p->K) return VIL_ERR_INVALID_ARGUMENT;
        for (int f = 0; f < p->n_edge; ++f) if (p->edge_pose[f] < 0 || p->edge_pose[f] >= p->K) return VIL_ERR_INVALID_ARGUMENT;
    }
    for (int f = 0; f < p->n_imu; ++f) if (p->imu_i[f] < 0 || p->imu_i[f] >= p->K || p->imu_j[f] < 0 || p->imu_j[f] >= p->K) return VIL_ERR_INVALID_ARGUMENT;
    for (int q = 0; q < 4 * p->n_icp; ++q) if (p->icp_ids[q] < 0 || p->icp_ids[q] >= p->K) return VIL_ERR_INVALID_ARGUMENT;
    for (int q = 0; q < 2 * p->n_lps; ++q) if (p->lps_ids[q] < 0 || p->lps_ids[q] >= p->K) return VIL_ERR_INVALID_ARGUMENT;
    if (p->prior.n > 0) {
        const vil_prior& pr = p->prior;
        if (pr.nblk <= 0 || !pr.blk_kind || !pr.blk_index || !pr.blk_col || (!win && (!pr.x0 || !pr.J0 || !pr.r0))) return VIL_ERR_INVALID_ARGUMENT;
        for (int b = 0; b < pr.nblk; ++b) {
            const int kind = pr.blk_kind[b], idx = pr.blk_index[b];
            if (kind < VIL_BLK_POSE || kind > VIL_BLK_TD) return VIL_ERR_INVALID_ARGUMENT;
            if ((kind == VIL_BLK_POSE || kind == VIL_BLK_SPEEDBIAS) && (idx < 0 || idx >= p->K)) return VIL_ERR_INVALID_ARGUMENT;
            if (pr.blk_col[b] < 0 || pr.blk_col[b] + blk_cols(kind) > pr.n) return VIL_ERR_INVALID_ARGUMENT;
        }
    }
    return VIL_OK;
}

// pose-sort LiDAR points, transpose to SoA (straight into `dst`, ncomp x stride doubles), build (start,count,pose) chunks of <= 256 points
static void lidar_order(int n, const int* pose, int K, std::vector<int>& perm, std::vector<int>& cnt) {
    perm.resize(n);
    cnt.assign(K + 1, 0);
    for (int f = 0; f < n; ++f) cnt[pose[f] + 1]++;
    for (int k = 0; k < K; ++k) cnt[k + 1] += cnt[k];
    std::vector<int> pos(cnt.begin(), cnt.end() - 1);
    for (int f = 0; f < n; ++f) perm[pos[pose[f]]++] = f;
}
static void lidar_soa(int n, int ncomp, const double* c, const std::vector<int>& perm, int stride, double* dst) {
    for (int q = 0; q < ncomp; ++q) {
        double* row = dst + (size_t)q * stride;
        for (int sidx = 0; sidx < n; ++sidx) row[sidx] = c[(size_t)perm[sidx] * ncomp + q];
        for (int sidx = n; sidx < stride; ++sidx) row[sidx] = 0.0;
    }
}
static void lidar_chunks(const std::vector<int>& cnt, int K, std::vector<int>& chunks) {
    chunks.clear();
    for (int k = 0; k < K; ++k) for (int s = cnt[k]; s < cnt[k + 1]; s += VIL_THREADS) { chunks.push_back(s); chunks.push_back(std::min(VIL_THREADS, cnt[k + 1] - s)); chunks.push_back(k); }
}

// ---- plan of the visual role (vil_sweep.hpp: sweep_visual), host logic without a device -------------------------------------------------------------
// The sweep walks the landmarks sorted by (first frame, last frame) -- insertion order in a tracker's feature list is already close to that -- and the
// factor tables are STORED in that order (sorted position <-> caller's factor: vfac / vfinv), so that a chunk's factors are consecutive rows of the SoA
// tables.  The sorted list is cut into chunks, one per workgroup, so that (a) a chunk fits the role's LDS (VIS_LM landmarks, VIS_MF factors, VIS_GM doubles of
// operand rows at the row stride of ITS window), (b) the matrix-core work of a chunk, (rows / 4) x tiles of its window, stays under a cap found by bisection:
// the smallest one that gives every chunk a compute unit of its own in the first round of the launch (vwg_max).  A chunk below VIL_VCHUNK_FBAL factors is
// not closed for balance (a workgroup's fixed cost is ~8 us whatever it holds).
struct VisPlan {
    std::vector<int> order, fperm, finv;                 // sorted landmarks (those with factors); sorted position -> caller's factor and back
    std::vector<int> vwg, vrec, vlm, vfac, wend;         // the device tables (vil_dev.hpp)
    size_t rec_doubles = 0; int n_chunks = 0, tmax = 1, gm = 0, cap = 0;
};
static bool plan_visual(const int K, const int L, const int n_vis, const std::vector<int>& lms, const std::vector<int>& fmin, const std::vector<int>& fmax, const std::vector<int>& anch,
                        const int vwg_max, const int cap_forced, VisPlan& o) {
    o.order.clear(); o.fperm.assign(std::max(n_vis, 1), 0); o.finv.assign(std::max(n_vis, 1), 0);
    {   // by (first frame, last frame, index): a counting sort over the K^2 frame pairs, stable in the index (a comparison sort of a tracker's ~1000 landmarks was 40 us of
        // every image's 110 us of host preparation)
        std::vector<int> cnt((size_t)K * K + 1, 0);
        int nlive = 0;
        for (int l = 0; l < L; ++l) if (lms[l + 1] > lms[l]) { ++cnt[(size_t)fmin[l] * K + fmax[l] + 1]; ++nlive; }
        for (size_t q = 0; q < (size_t)K * K; ++q) cnt[q + 1] += cnt[q];
        o.order.assign(nlive, 0);
        for (int l = 0; l < L; ++l) if (lms[l + 1] > lms[l]) o.order[cnt[(size_t)fmin[l] * K + fmax[l]]++] = l;
    }
    { int pos = 0; for (int l : o.order) for (int f = lms[l]; f < lms[l + 1]; ++f) { o.fperm[pos] = f; o.finv[f] = pos; ++pos; } }
    const std::vector<int>& order = o.order;
    struct Chunk { int p0, nl, nf, fa, span; };
    std::vector<Chunk> ch;
    auto cost = [](int nf, int T) { return (vd::vis_rows(nf) / 4 + 4) * vd::vis_ntile(T); };
    auto cut = [&](int cap) -> bool {
        ch.clear();
        Chunk cc{0, 0, 0, 0, 0}; int wlo = K, whi = -1;
        for (int q = 0; q < (int)order.size(); ++q) {
            const int l = order[q], n = lms[l + 1] - lms[l];
            const int lo = std::min(wlo, fmin[l]), hi = std::max(whi, fmax[l]), T = vd::vis_tiles(hi - lo + 1);
            const bool fits = cc.nl < VIS_LM && cc.nf + n <= VIS_MF && vd::vis_gm_doubles(cc.nf + n, T) <= VIS_GM;
            if (cc.nl > 0 && (!fits || (cc.nf >= VIL_VCHUNK_FBAL && cost(cc.nf + n, T) > cap))) {
                cc.fa = wlo; cc.span = whi - wlo + 1; ch.push_back(cc);
                cc = Chunk{q, 0, 0, 0, 0}; wlo = K; whi = -1;
            }
            if (cc.nl == 0 && (n > VIS_MF || vd::vis_gm_doubles(n, vd::vis_tiles(fmax[l] - fmin[l] + 1)) > VIS_GM)) return false;      // a landmark no chunk can hold
            cc.nl++; cc.nf += n; wlo = std::min(wlo, fmin[l]); whi = std::max(whi, fmax[l]);
        }
        if (cc.nl > 0) { cc.fa = wlo; cc.span = whi - wlo + 1; ch.push_back(cc); }
        return true;
    };
    int lo = cost(VIL_VCHUNK_FBAL, 1), hi = cost(VIS_MF, VIS_TMAX);
    if (cap_forced > 0) lo = hi = cap_forced;
    if (!cut(lo)) return false;
    o.cap = lo;
    if ((int)ch.size() > vwg_max) {
        while (lo < hi) { const int mid = (lo + hi) / 2; cut(mid); if ((int)ch.size() <= vwg_max) hi = mid; else lo = mid + 1; }
        cut(hi); o.cap = hi;
    }
    const int nw = (int)ch.size();
    o.n_chunks = nw;
    o.vwg.assign(8 * (size_t)std::max(nw, 1), 0); o.vrec.assign(4 * (size_t)std::max(nw, 1), 0); o.vlm.assign(4 * std::max(order.size(), (size_t)1), 0); o.vfac.assign(2 * (size_t)std::max(n_vis, 1), 0);
    size_t roff = 0; int fpos = 0;
    o.tmax = 1; o.gm = 0;
    for (int w = 0; w < nw; ++w) {
        const Chunk& cc = ch[w];
        const int T = vd::vis_tiles(cc.span);
        int* d = &o.vwg[8 * (size_t)w];
        d[0] = cc.p0; d[1] = cc.nl; d[2] = fpos; d[3] = cc.nf; d[4] = cc.fa; d[5] = cc.span; d[6] = T; d[7] = (int)(roff / 16);
        int* r = &o.vrec[4 * (size_t)w]; r[0] = d[7]; r[1] = cc.fa; r[2] = cc.span; r[3] = T;
        int floc = 0;
        for (int q = 0; q < cc.nl; ++q) {
            const int l = order[cc.p0 + q], n = lms[l + 1] - lms[l];
            int* e = &o.vlm[4 * (size_t)(cc.p0 + q)]; e[0] = l; e[1] = floc; e[2] = n; e[3] = anch[l];
            for (int k = 0; k < n; ++k) { o.vfac[2 * (size_t)(fpos + floc + k)] = lms[l] + k; o.vfac[2 * (size_t)(fpos + floc + k) + 1] = q; }
            floc += n;
        }
        fpos += cc.nf; roff += (size_t)vd::vis_rec_doubles(T);
        o.tmax = std::max(o.tmax, T); o.gm = std::max(o.gm, vd::vis_gm_doubles(cc.nf, T));
    }
    o.rec_doubles = roff;
    o.wend.assign(std::max(K, 1), 0);
    for (int w = 0; w < nw; ++w) for (int f = ch[w].fa; f < K; ++f) o.wend[f]++;
    return true;
}
// frame range and anchor of every landmark from the caller's factor tables
static void landmark_frames(const vil_problem* p, std::vector<int>& lms, std::vector<int>& fmin, std::vector<int>& fmax, std::vector<int>& anch) {
    const int L = p->L, K = p->K;
    lms.assign(L + 1, 0); fmin.assign(std::max(L, 1), K); fmax.assign(std::max(L, 1), -1); anch.assign(std::max(L, 1), 0);
    for (int f = 0; f < p->n_vis; ++f) lms[p->vis_l[f] + 1]++;
    for (int l = 0; l < L; ++l) lms[l + 1] += lms[l];
    for (int f = 0; f < p->n_vis; ++f) {
        const int l = p->vis_l[f], lo = std::min(p->vis_i[f], p->vis_j[f]), hi = std::max(p->vis_i[f], p->vis_j[f]);
        anch[l] = p->vis_i[f]; fmin[l] = std::min(fmin[l], lo); fmax[l] = std::max(fmax[l], hi);
    }
}
// helper workgroups of the step kernel for L landmarks: none below one landmark per master thread, else one per 128 (quad of lanes per landmark) or 256 (pair) landmarks, at most 15
// (a helper keeps its landmarks' rows in registers between its two passes while it has at least one thread per landmark -- vil_step.hpp, lm_rows_quad:
//  up to 1920 landmarks a QUAD of threads per landmark, 128 landmarks per helper; beyond that a PAIR, 256 per helper; at most 15 helpers, so past
//  3840 landmarks a helper's threads loop over its slice)
// Master and helpers wait for one another inside the launch: all of them must be resident at once (vil_coop.hpp).  With its dynamic LDS a step workgroup
// owns a compute unit; a device with fewer units than 1 + n_help runs without helpers.
static int vil_helpers_for(int L, int device) {
    const int quad = VIL_STEP_THREADS / 4, pair = VIL_STEP_THREADS / 2;
    int n = L < VIL_STEP_THREADS ? 0 : std::min(15, L <= 15 * quad ? (L + quad - 1) / quad : (L + pair - 1) / pair);
    if (const char* ev = VIL_TUNE_ENV("VIL_HELP")) n = std::max(0, std::min(15, atoi(ev)));
    if (1 + n > vilcoop::compute_units(device) / 2) n = 0;      // (what this process really has: a CU mask is not in the device attribute)
    return n;
}
// Co-residency is decided per XCD: the dispatcher deals the workgroups of a grid round-robin to the eight XCDs, each of which places ITS share on ITS compute units.
// n consecutive workgroups that wait for others therefore need ceil(n / 8) slots on every XCD, and one more for the workgroups they wait for to run through
// (measured under a 32-unit mask, 4 units per XCD: 25 waiting workgroups fit the device's 32 slots and still starved the gather workgroups of one XCD).
static bool fits_per_xcd(int n_resident, int capacity) { return (n_resident + 7) / 8 + 1 <= capacity / 8; }
static int visual_wg_budget(int n_imu, int n_plane, int n_edge) { return std::max(64, 256 - (n_imu + 3 + (n_plane + 511) / 512 + (n_edge + 511) / 512)); }
// diagnostic surface of the plan (no device needed: the CPU test suite checks its invariants; DESIGN.md quotes its record sizes)
int vil_visual_plan(const vil_problem* p, vil_visual_plan_info* info, int32_t max_chunks, int32_t* chunk_first_frame, int32_t* chunk_frames, int32_t* chunk_factors, int32_t* chunk_landmarks,
                    int32_t* factor_position) {
    if (!p || !info) return VIL_ERR_INVALID_ARGUMENT;
    for (int f = 0; f < p->n_vis; ++f) {
        if (!p->vis_l || !p->vis_i || !p->vis_j || p->vis_l[f] < 0 || p->vis_l[f] >= p->L || p->vis_i[f] < 0 || p->vis_i[f] >= p->K || p->vis_j[f] < 0 || p->vis_j[f] >= p->K) return VIL_ERR_INVALID_ARGUMENT;
        if (f && p->vis_l[f] < p->vis_l[f - 1]) return VIL_ERR_INVALID_ARGUMENT;
    }
    std::vector<int> lms, fmin, fmax, anch;
    landmark_frames(p, lms, fmin, fmax, anch);
    VisPlan vp;
    if (!plan_visual(p->K, p->L, p->n_vis, lms, fmin, fmax, anch, visual_wg_budget(p->n_imu, std::max(p->n_plane, 0), std::max(p->n_edge, 0)), 0, vp)) return VIL_ERR_UNSUPPORTED;
    memset(info, 0, sizeof *info);
    info->n_chunks = vp.n_chunks; info->max_tiles = vp.tmax; info->tiles_per_wave = vd::vis_slots(vp.tmax) <= 2 ? 2 : 5; info->cost_cap = vp.cap;
    info->record_bytes = (int64_t)(8 * vp.rec_doubles); info->lds_bytes = (int64_t)(8 * (size_t)(VIS_LDS_FIXED + vp.gm));
    info->dense_record_bytes = (int64_t)vp.n_chunks * 8 * ((6 * p->K + 7) * (6 * p->K + 8) / 2 + 3 * (6 * p->K + 7) + 1);
    for (int w = 0; w < vp.n_chunks && w < max_chunks; ++w) {
        if (chunk_first_frame) chunk_first_frame[w] = vp.vwg[8 * (size_t)w + 4];
        if (chunk_frames) chunk_frames[w] = vp.vwg[8 * (size_t)w + 5];
        if (chunk_factors) chunk_factors[w] = vp.vwg[8 * (size_t)w + 3];
        if (chunk_landmarks) chunk_landmarks[w] = vp.vwg[8 * (size_t)w + 1];
    }
    if (factor_position) for (int f = 0; f < p->n_vis; ++f) factor_position[f] = vp.finv[f];
    return VIL_OK;
}


// gp / vis_f0 (sharded): the whole window's problem and the index of this rank's first visual factor in it
// Resident sources of the big tables (vil_win_solve): the visual factor tables are expanded on the device from the landmark
// list + observation store, IMU records / sqrt-information come from the IMU slots, the prior is the device prior slot (WinSlots: what Window::fill
// sets).  The vil_problem handed to upload_impl then carries n_vis = 0, imu_const = NULL and the prior's block tables only.
struct WinSrc : WinSlots {
    const int* lm_track; const int* lm_startf; const int* lm_nobs;      // host, L each
    int n_vis;
    int lb, le, f0, n_vis_all;       // sharded (gp != null): this rank keeps the factors of landmarks [lb, le), the first of which is factor f0 of the n_vis_all of the window
};

// ---- upload_impl, stage by stage.  Every table goes into ONE pinned image in the order of its put(): the arena layout is that order.
struct ImageBuilder {
    Arena& ar;
    struct Fix { size_t off; void** slot; bool scratch; };
    std::vector<Fix> fix;          // slots patched with the device address once the arena is allocated (commit)
    bool oom = false;
    // src != null: a table (copied into the pinned image); src == null: zero-initialised device work space
    void put(const void* src, size_t bytes, void** slot) {
        if (!src || !bytes) fix.push_back({ar.take_scratch(bytes ? bytes : 8), slot, true});
        else if (char* h = reserve(bytes, slot)) memcpy(h, src, bytes);
    }
    // a table that is produced in place (transpositions): space in the pinned image, to be filled before the next put()
    char* reserve(size_t bytes, void** slot) {
        const size_t o = ar.take(bytes ? bytes : 8);
        if (o == (size_t)-1) { oom = true; return nullptr; }
        fix.push_back({o, slot, false});
        return ar.h.p + o;
    }
};
// the parameter block's header, constancy, state x[0], x[1] and its backups
static void upload_state(vil_ctx* c, ImageBuilder& im, const vil_problem* p, const vil_state* s, const WinSrc* ws, DevP& P) {
    const int K = p->K, L = p->L, NS = 16 * K + 8 + L;
    P.K = K; P.L = L; P.D = 15 * K + 7; P.NV = 6 * K + 7; P.NS = NS;
    P.ex_const = p->ex_const; P.use_td = p->use_td; P.td_free = (p->use_td && !p->td_const) ? 1 : 0;
    memcpy(P.G, p->G, sizeof P.G); P.sqrt_info = p->sqrt_info_px; P.k_tr = p->tr_over_row;
    { double R[9]; quat_to_R_host(p->q_lb, R); for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) P.Rbl[3 * i + j] = R[3 * j + i]; }
      for (int i = 0; i < 3; ++i) P.tbl[i] = -(P.Rbl[3 * i] * p->t_lb[0] + P.Rbl[3 * i + 1] * p->t_lb[1] + P.Rbl[3 * i + 2] * p->t_lb[2]); }
    if (p->pose_const) im.put(p->pose_const, K, (void**)&P.pose_const);
    if (p->sb_const) im.put(p->sb_const, K, (void**)&P.sb_const);
    if (p->lm_const && L) im.put(p->lm_const, L, (void**)&P.lm_const);
    std::vector<double> x(NS);
    memcpy(&x[0], s->pose, sizeof(double) * 7 * K); memcpy(&x[7 * K], s->speedbias, sizeof(double) * 9 * K);
    memcpy(&x[16 * K], s->ex_pose, sizeof(double) * 7); x[16 * K + 7] = s->td[0];
    if (L) memcpy(&x[16 * K + 8], s->inv_depth, sizeof(double) * L);
    im.put(x.data(), sizeof(double) * NS, (void**)&P.x[0]);
    if (ws) { im.put(nullptr, sizeof(double) * NS, (void**)&P.x[1]); im.put(nullptr, sizeof(double) * NS, (void**)&c->d_x0); }      // (k_win_pack copies them on the device)
    else { im.put(x.data(), sizeof(double) * NS, (void**)&P.x[1]); im.put(x.data(), sizeof(double) * NS, (void**)&c->d_x0); }
    im.put(nullptr, sizeof(double) * NS, (void**)&c->d_xsave);
}
// visual tables, sorted and cut into chunks by plan_visual; wd_track / wd_startf: device copies of the landmark table (resident window)
static int upload_visual(vil_ctx* c, ImageBuilder& im, const vil_problem* p, const WinSrc* ws, const vil_problem* gp, int vis_f0, DevP& P, int** wd_track, int** wd_startf) {
    const int K = p->K, L = p->L, n_vis = ws ? ws->n_vis : p->n_vis;
    P.n_vis = n_vis; P.vis_stride = (n_vis + 31) & ~31;
    // factor prefix, frame window and anchor of every landmark, then the plan of the visual role (plan_visual above: sorted order, chunks, device tables)
    std::vector<int> lms, fmin, fmax, anch;
    if (ws) {
        const int ws_lb = gp ? ws->lb : 0, ws_le = gp ? ws->le : L;      // resident window under a communicator: the factors of the owned landmarks only
        lms.assign(L + 1, 0); fmin.assign(std::max(L, 1), K); fmax.assign(std::max(L, 1), -1); anch.assign(std::max(L, 1), 0);
        for (int l = 0; l < L; ++l) lms[l + 1] = lms[l] + ((l >= ws_lb && l < ws_le) ? ws->lm_nobs[l] - 1 : 0);
        for (int l = ws_lb; l < ws_le; ++l) { anch[l] = fmin[l] = ws->lm_startf[l]; fmax[l] = ws->lm_startf[l] + ws->lm_nobs[l] - 1; }
    } else landmark_frames(p, lms, fmin, fmax, anch);
    VisPlan vp;
    int npt = std::max(p->n_plane, 0), net = std::max(p->n_edge, 0);           // LiDAR points of this upload (resident slabs: what they hold)
    if (p->n_plane == VIL_LIDAR_RESIDENT) c->lidar.totals(&npt, &net);
    int vwg_max = visual_wg_budget(p->n_imu, npt, net), cap_forced = 0;
    if (const char* ev = VIL_TUNE_ENV("VIL_VWG")) vwg_max = std::max(1, atoi(ev));
    if (const char* ev = VIL_TUNE_ENV("VIL_VCAP")) cap_forced = std::max(1, atoi(ev));
    if (!plan_visual(K, L, n_vis, lms, fmin, fmax, anch, vwg_max, cap_forced, vp)) return VIL_ERR_UNSUPPORTED;
    const std::vector<int>& fperm = vp.fperm; const std::vector<int>& finv = vp.finv;
    im.put(finv.data(), 4 * finv.size(), (void**)&P.vfinv);
    if (ws) {
        // resident window: the factor tables are device work space, k_win_pack fills them from the observation store
        im.put(nullptr, 8 * (size_t)14 * std::max(P.vis_stride, 1), (void**)&P.vis_c);
        im.put(nullptr, 4 * (size_t)std::max(n_vis, 1), (void**)&P.vis_i); im.put(nullptr, 4 * (size_t)std::max(n_vis, 1), (void**)&P.vis_j); im.put(nullptr, 4 * (size_t)std::max(n_vis, 1), (void**)&P.vis_l);
        im.put(ws->lm_track, 4 * (size_t)std::max(L, 1), (void**)wd_track); im.put(ws->lm_startf, 4 * (size_t)std::max(L, 1), (void**)wd_startf);
    } else {
        if (double* soa = (double*)im.reserve(8 * (size_t)14 * std::max(P.vis_stride, 1), (void**)&P.vis_c)) {
            for (int q = 0; q < 14; ++q) {
                double* row = soa + (size_t)q * P.vis_stride;
                for (int pos = 0; pos < p->n_vis; ++pos) row[pos] = p->vis_const[(size_t)fperm[pos] * 14 + q];
                for (int f = p->n_vis; f < P.vis_stride; ++f) row[f] = 0.0;
            }
        }
        std::vector<int> si(std::max(p->n_vis, 1)), sj(std::max(p->n_vis, 1)), sl(std::max(p->n_vis, 1));
        for (int pos = 0; pos < p->n_vis; ++pos) { si[pos] = p->vis_i[fperm[pos]]; sj[pos] = p->vis_j[fperm[pos]]; sl[pos] = p->vis_l[fperm[pos]]; }
        im.put(si.data(), 4 * (size_t)p->n_vis, (void**)&P.vis_i); im.put(sj.data(), 4 * (size_t)p->n_vis, (void**)&P.vis_j); im.put(sl.data(), 4 * (size_t)p->n_vis, (void**)&P.vis_l);
    }
    im.put(lms.data(), 4 * (size_t)(L + 1), (void**)&P.lm_start);
    std::vector<int> acol(std::max(L, 1), -1);
    if (ws) {
        for (int l = 0; l < L; ++l) acol[l] = 6 * ws->lm_startf[l];
        im.put(acol.data(), 4 * acol.size(), (void**)&P.lm_acol); im.put(nullptr, 4 * (size_t)std::max(n_vis, 1), (void**)&P.fcol);
    } else {
        std::vector<int> fcol(std::max(p->n_vis, 1), 0);
        for (int f = p->n_vis - 1; f >= 0; --f) { acol[p->vis_l[f]] = 6 * p->vis_i[f]; fcol[f] = 6 * p->vis_j[f]; }
        im.put(acol.data(), 4 * acol.size(), (void**)&P.lm_acol); im.put(fcol.data(), 4 * fcol.size(), (void**)&P.fcol);
    }
    if (gp) {                                        // tables of the whole window for the step kernel (every rank walks every landmark)
        const int gnv = ws ? ws->n_vis_all : gp->n_vis;
        std::vector<int> gl(L + 1, 0), gac(std::max(L, 1), -1), gfc(std::max(gnv, 1), 0);
        if (ws) {
            for (int l = 0; l < L; ++l) {
                gl[l + 1] = gl[l] + ws->lm_nobs[l] - 1; gac[l] = 6 * ws->lm_startf[l];
                for (int q = 1; q < ws->lm_nobs[l]; ++q) gfc[gl[l] + q - 1] = 6 * (ws->lm_startf[l] + q);
            }
        } else {
            for (int f = 0; f < gp->n_vis; ++f) gl[gp->vis_l[f] + 1]++;
            for (int l = 0; l < L; ++l) gl[l + 1] += gl[l];
            for (int f = gp->n_vis - 1; f >= 0; --f) { gac[gp->vis_l[f]] = 6 * gp->vis_i[f]; gfc[f] = 6 * gp->vis_j[f]; }
        }
        im.put(gl.data(), 4 * gl.size(), (void**)&P.glm_start); im.put(gac.data(), 4 * gac.size(), (void**)&P.glm_acol); im.put(gfc.data(), 4 * gfc.size(), (void**)&P.gfcol);
        P.vis_f0 = vis_f0;
    }
    P.n_vwg = vp.n_chunks;
    P.vis_ts = vd::vis_slots(vp.tmax) <= 2 ? 2 : 5;
    c->vis_gm = vp.gm;
    im.put(vp.wend.data(), 4 * vp.wend.size(), (void**)&P.vwend);
    im.put(vp.vwg.data(), 4 * vp.vwg.size(), (void**)&P.vwg); im.put(vp.vrec.data(), 4 * vp.vrec.size(), (void**)&P.vrec);
    im.put(vp.vlm.data(), 4 * vp.vlm.size(), (void**)&P.vlm); im.put(vp.vfac.data(), 4 * vp.vfac.size(), (void**)&P.vfac);
#ifdef VIL_TUNING
    im.put(nullptr, 8 * 2 * std::max(vp.rec_doubles, (size_t)16), (void**)&P.vpart);      // (x 2: the second half is the mirror of the record-traffic experiment, VIL_SKIP=1024 -- tuning build only)
    P.vmirror = (long long)std::max(vp.rec_doubles, (size_t)16);
#else
    im.put(nullptr, 8 * std::max(vp.rec_doubles, (size_t)16), (void**)&P.vpart);
#endif
    return VIL_OK;
}
// LiDAR tables: the caller's points pose-sorted into SoA, or only the chunk lists (device-resident points, the context's slabs)
static int upload_lidar(vil_ctx* c, ImageBuilder& im, const vil_problem* p, const vil_device_lidar* dl, DevP& P) {
    const int K = p->K;
    std::vector<int> ch, cnt;
    std::vector<int> lcp(2 * (K + 1), 0);   // chunk ranges per pose (chunks are pose-ordered): plane [0..K], edge [K+1..2K+1]
    const bool res_lidar = p->n_plane == VIL_LIDAR_RESIDENT && p->n_edge == VIL_LIDAR_RESIDENT;
    c->lidar_resident = res_lidar;
    // one kind of point factor (plane: 7 components, edge: 9): its chunk list, and for the caller's points the pose-sorted SoA table.  Only the chunk list for
    // device-resident tables (vil_internal.h: every factor sits on pose 0 in the caller's order) and resident frame slabs (vil_lidar_push: slab i belongs to pose K - count + i)
    auto kind = [&](bool plane, int n, const int* pose, const double* cst, std::vector<int>& perm, const double** soa, int* stride, int* nchunk, const int** tab, int base) {
        const int ncomp = plane ? 7 : 9;
        ch.clear(); perm.clear();
        if (res_lidar) c->lidar.chunks(plane, K, ch);
        else if (dl) for (int s0 = 0; s0 < n; s0 += VIL_THREADS) { ch.push_back(s0); ch.push_back(std::min(VIL_THREADS, n - s0)); ch.push_back(0); }
        if (res_lidar || dl) im.put(nullptr, 8, (void**)soa);
        else {
            lidar_order(n, pose, K, perm, cnt); lidar_chunks(cnt, K, ch);
            *stride = (n + 31) & ~31;
            if (double* dst = (double*)im.reserve(8 * (size_t)ncomp * std::max(*stride, 1), (void**)soa)) lidar_soa(n, ncomp, cst, perm, *stride, dst);
        }
        *nchunk = (int)ch.size() / 3;
        for (size_t q = 0; q < ch.size() / 3; ++q) { lcp[base + ch[3 * q + 2] + 1]++; if (ch[3 * q + 2] == 0) c->mm.lidar0 = true; }
        for (int k = 0; k < K; ++k) lcp[base + k + 1] += lcp[base + k];
        im.put(ch.data(), 4 * ch.size(), (void**)tab);
    };
    if (res_lidar && c->lidar.count() > K) return VIL_ERR_UNSUPPORTED;
    c->mm.lidar0 = false;
    kind(true, p->n_plane, p->plane_pose, p->plane_const, c->plane_perm, &P.pl_c, &P.pl_stride, &P.n_pchunk, &P.pchunk, 0);
    kind(false, p->n_edge, p->edge_pose, p->edge_const, c->edge_perm, &P.ed_c, &P.ed_stride, &P.n_echunk, &P.echunk, K + 1);
    P.n_plane = p->n_plane; P.n_edge = p->n_edge;
    if (res_lidar) c->lidar.totals(&P.n_plane, &P.n_edge);
    // (resident slabs under a communicator: a frame with fewer points than ranks leaves some ranks' slices empty -- whether pose 0 carries LiDAR factors, and with it the
    //  kept / dropped layout of the marginalisation every rank commits, is decided from the UNSLICED counts)
    if (res_lidar) c->mm.lidar0 = c->lidar.frame0_has_points(K);
    im.put(nullptr, 8 * (size_t)28 * std::max(P.n_pchunk + P.n_echunk, 1), (void**)&P.lpart);
    im.put(lcp.data(), 4 * lcp.size(), (void**)&P.lchunk_pose);
    return VIL_OK;
}
// IMU, prior and ICP / LPS tables; pinv: reduced-system column -> prior column (-1: none)
static int upload_imu_prior(vil_ctx* c, ImageBuilder& im, const vil_problem* p, const WinSrc* ws, DevP& P, std::vector<int>& pinv) {
    const int K = p->K, D = 15 * K + 7;
    P.n_imu = p->n_imu;
    if (ws) im.put(nullptr, 8 * (size_t)287 * std::max(p->n_imu, 1), (void**)&P.imu_c);      // gathered from the IMU slots by k_win_pack, like U
    else im.put(p->imu_const, 8 * (size_t)287 * p->n_imu, (void**)&P.imu_c);
    im.put(nullptr, 8 * (size_t)225 * std::max(p->n_imu, 1), (void**)&P.imu_U);
    im.put(p->imu_i, 4 * (size_t)p->n_imu, (void**)&P.imu_i); im.put(p->imu_j, 4 * (size_t)p->n_imu, (void**)&P.imu_j);
    im.put(nullptr, 8 * (size_t)931 * std::max(p->n_imu, 1), (void**)&P.ipart);
    if (!c->d_imu_perm.p) {   // the order of an IMU role's record entries in a one-launch iteration: what the chain workgroup gathers first.  Constant: one device copy per context
        int perm[1024]; int n = VIL_CHAIN_REC;
        for (int e = 0; e < 931; ++e) { const int ce = chain_rec_index(e); if (ce >= 0) perm[ce] = e; else perm[n++] = e; }
        for (int e = 931; e < 1024; ++e) perm[e] = 930;
        HIPCHK(c->d_imu_perm.reserve(1024, 1024));
        HIPCHK(hipMemcpy(c->d_imu_perm.p, perm, sizeof(perm), hipMemcpyHostToDevice));
    }
    P.imu_perm = c->d_imu_perm.p;
    im.put(nullptr, 4 * (size_t)(std::max(p->n_imu, 1) + 8), (void**)&P.cflag);
    im.put(nullptr, 8 * (size_t)VIL_CHAIN_REC * std::max(p->n_imu, 1), (void**)&P.irec);      // (compact IMU records for the chain workgroup of a one-launch iteration)
    P.pn = p->prior.n > 0 ? p->prior.n : 0; P.pnblk = P.pn ? p->prior.nblk : 0;
    c->prior_joff.clear();
    pinv.assign(D, -1);
    if (P.pn) {
        const vil_prior& pr = p->prior;
        const int n = pr.n;
        std::vector<int> xoff(pr.nblk), pmap(n, -1);
        int xo = 0, jo = 0;
        for (int b = 0; b < pr.nblk; ++b) {
            const int kind = pr.blk_kind[b], gs = blk_doubles(kind), ls = blk_cols(kind);
            xoff[b] = xo; xo += gs; c->prior_joff.push_back(jo); jo += n * gs;
            int col = -1;
            const int idx = pr.blk_index[b];
            if (kind == VIL_BLK_POSE) { if (idx < 0 || idx >= K) return VIL_ERR_INVALID_ARGUMENT; col = (p->pose_const && p->pose_const[idx]) ? -1 : 6 * idx; }
            else if (kind == VIL_BLK_SPEEDBIAS) { if (idx < 0 || idx >= K) return VIL_ERR_INVALID_ARGUMENT; col = (p->sb_const && p->sb_const[idx]) ? -1 : 6 * K + 7 + 9 * idx; }
            else if (kind == VIL_BLK_EX) col = p->ex_const ? -1 : 6 * K;
            else col = P.td_free ? 6 * K + 6 : -1;
            if (pr.blk_col[b] < 0 || pr.blk_col[b] + ls > n) return VIL_ERR_INVALID_ARGUMENT;
            for (int q = 0; q < ls; ++q) pmap[pr.blk_col[b] + q] = col < 0 ? -1 : col + q;
        }
        im.put(pr.blk_kind, 4 * (size_t)pr.nblk, (void**)&P.pblk_kind); im.put(pr.blk_index, 4 * (size_t)pr.nblk, (void**)&P.pblk_index);
        im.put(pr.blk_col, 4 * (size_t)pr.nblk, (void**)&P.pblk_col); im.put(xoff.data(), 4 * (size_t)pr.nblk, (void**)&P.pblk_xoff);
        im.put(pmap.data(), 4 * (size_t)n, (void**)&P.pmap);
        for (int q = 0; q < n; ++q) if (pmap[q] >= 0) pinv[pmap[q]] = q;
        if (!ws) {
            im.put(pr.x0, 8 * (size_t)xo, (void**)&P.px0); im.put(pr.J0, 8 * (size_t)n * n, (void**)&P.pJ0); im.put(pr.r0, 8 * (size_t)n, (void**)&P.pr0);
            im.put(nullptr, 8 * (size_t)n * n, (void**)&P.pH); im.put(nullptr, 8 * (size_t)n, (void**)&P.pg0); im.put(nullptr, 8, (void**)&P.pc0);
        }
    }
    im.put(pinv.data(), 4 * (size_t)D, (void**)&P.pinv);
    im.put(nullptr, 8 * (size_t)((P.pn ? P.pn + 1 : 0) + 601 * (p->n_icp + p->n_lps) + 1), (void**)&P.mpart);
    P.n_icp = p->n_icp; P.n_lps = p->n_lps;
    im.put(p->icp_ids, 16 * (size_t)p->n_icp, (void**)&P.icp_ids); im.put(p->icp_const, 80 * (size_t)p->n_icp, (void**)&P.icp_c);
    im.put(p->lps_ids, 8 * (size_t)p->n_lps, (void**)&P.lps_ids); im.put(p->lps_const, 56 * (size_t)p->n_lps, (void**)&P.lps_c);
    return VIL_OK;
}
// systems + work space (zero-initialised); returns the doubles of a system set's camera part
static size_t upload_workspace(vil_ctx* c, ImageBuilder& im, const WinSrc* ws, const vil_problem* gp, bool sharded, DevP& P) {
    const int K = P.K, L = P.L, D = P.D, NV = P.NV;
    // one contiguous block per set: [S | gred | bc | diag | cost | 2 spare | hll | bl | invp | sl | eA | eO]
    const size_t Lp = (size_t)std::max(L, 1), Fp = (size_t)std::max(gp ? (ws ? ws->n_vis_all : gp->n_vis) : P.n_vis, 1);
    const size_t ar_cam = ((size_t)D * D + 3 * (size_t)D + 3 + 1) & ~size_t(1);
    c->span = ar_cam + 4 * Lp + 13 * Lp + 6 * Fp;
    for (int q = 0; q < 2; ++q) im.put(nullptr, 8 * c->span, (void**)&P.sys[q].ar);
    P.rank = sharded ? c->comm.rank : 0; P.world = sharded ? c->comm.world : 1;
    for (auto& g : c->graphs) hipGraphExecDestroy(g.exec);
    c->graphs.clear(); c->solves_since_upload = 0;
    c->sharded = sharded && c->comm.world > 1;
    // multi-GPU plumbing (set 0 = this rank's partial system, all-reduced into set 1, which the step kernel reads); vil_debug_set_split
    // runs it on a single rank (tests)
    c->split = c->sharded || c->force_split;
    im.put(nullptr, 8 * (size_t)std::max(L, 1), (void**)&P.Sl); im.put(nullptr, 8 * (size_t)D, (void**)&P.Sc); im.put(nullptr, 8 * (size_t)D, (void**)&P.dc); im.put(nullptr, 8 * (size_t)std::max(L, 1), (void**)&P.dl);
    im.put(nullptr, 8 * (size_t)D, (void**)&P.gradc); im.put(nullptr, 8 * (size_t)std::max(L, 1), (void**)&P.gradl); im.put(nullptr, 8 * (size_t)D, (void**)&P.gnc); im.put(nullptr, 8 * (size_t)std::max(L, 1), (void**)&P.gnl);
    { const size_t Tm = (size_t)(D + 16) / 16; im.put(nullptr, 8 * std::max((size_t)D * D, (size_t)TILE_SZ * (Tm * (Tm + 1) / 2)), (void**)&P.M); } im.put(nullptr, 16 * (size_t)D, (void**)&P.stepc);      // (two 64-bit words per value: half + launch epoch)
    im.put(nullptr, 8 * 4 * 16, (void**)&P.hpart); im.put(nullptr, 4 * 16, (void**)&P.hflag);
    im.put(nullptr, 8 * 8 * 16 * 8, (void**)&P.hpart2); im.put(nullptr, 4 * 16 * 8, (void**)&P.hflag2);      // one slot per helper WAVE
    im.put(nullptr, 16, (void**)&P.xflag); im.put(nullptr, 16, (void**)&P.xstat);
    im.put(nullptr, 8 * (size_t)std::max(L, 1), (void**)&P.la); im.put(nullptr, 8 * (size_t)std::max(L, 1), (void**)&P.lb); im.put(nullptr, 8 * (size_t)std::max(L, 1), (void**)&P.stepl);
    im.put(nullptr, 8 * (size_t)D, (void**)&P.tmpc); im.put(nullptr, 8 * (size_t)std::max(L, 1), (void**)&P.tmpl);
    im.put(nullptr, sizeof(Ctl), (void**)&P.ctl);
    im.put(nullptr, 8 * 64, (void**)&P.dbg);
    im.put(nullptr, 8 * (size_t)vd::chain_wcols(K) * vd::chain_rs(K), (void**)&P.chW);      // (the chain eliminated ahead of the step kernel: chain_table)
    im.put(nullptr, 8 * (size_t)54 * K, (void**)&P.chLdg); im.put(nullptr, 8 * (size_t)82 * K, (void**)&P.chLsb); im.put(nullptr, 8 * (size_t)136 * K, (void**)&P.chLraw);
    im.put(nullptr, 8 * (size_t)9 * K, (void**)&P.chSc); im.put(nullptr, 8 * (size_t)9 * K, (void**)&P.chDc);
    im.put(nullptr, 8 * (size_t)2 * (NV + 1), (void**)&P.chZ); im.put(nullptr, 8 * 4, (void**)&P.chQ); im.put(nullptr, 16, (void**)&P.chOk);
    im.put(nullptr, 4 * (size_t)(gather_blocks(D, NV, RED_EPW, false) + 8), (void**)&P.gflag);      // (one flag per gather workgroup of the merged launch: never more than the gather kernel has)
    im.put(nullptr, 64, (void**)&P.chflag); im.put(nullptr, 4 * 64, (void**)&P.wwflag); im.put(nullptr, 4 * (size_t)(K + 8), (void**)&P.swflag);
    im.put(nullptr, 4 * 64, (void**)&P.sall);
    im.put(nullptr, 4 * (size_t)VIL_SFLAG_MAX, (void**)&P.sflag);      // one flag per sweep workgroup of a one-launch iteration (taken only when there are fewer: below)
    im.put(nullptr, 256, (void**)&P.ihdr); im.put(nullptr, 8 * 2 * (size_t)(16 * K + 8), (void**)&P.xtag);
    im.put(nullptr, 64, (void**)&P.abortf);      // (raised by a wait on another workgroup's flag that gives up: vil_math.hpp, spin_until_eq)
    { const size_t Tp = (size_t)(NV + 1 + 15) / 16; im.put(nullptr, 8 * (size_t)TILE_SZ * (Tp * (Tp + 1) / 2), (void**)&P.chWW); }
    im.put(nullptr, 8 * (size_t)VIL_CHC_MAX, (void**)&P.chc);
    return ar_cam;
}
// ---- chain eliminated ahead of the step kernel (vil_prechain.hpp): every IMU factor joins frames (k, k+1), at most one per pair, single GPU.
//      The gather table is built here once per upload: the chain workgroup then sums <= 3 sources per entry in a fixed order.  built: a new table went up.
static int chain_table(vil_ctx* c, const vil_problem* p, bool sharded, DevP& P, const std::vector<int>& pinv, bool& pre_ok, bool& built) {
    const int K = P.K, L = P.L, D = P.D, NV = P.NV;
    pre_ok = !sharded && !c->force_split && c->launch_mode != 2 && L >= 0 && K >= 3 && VIL_TUNE_ENV("VIL_NO_PRECHAIN") == nullptr;
    std::vector<int> as_i(K, -1), as_j(K, -1);
    for (int f = 0; f < p->n_imu && pre_ok; ++f) {
        const int i = p->imu_i[f], j = p->imu_j[f];
        if (j != i + 1 || as_i[i] >= 0 || as_j[j] >= 0) pre_ok = false; else { as_i[i] = f; as_j[j] = f; }
    }
    if (!pre_ok) return VIL_OK;
    // the table depends on K, the IMU factor layout and the prior's block structure only: consecutive windows of a tracker share it, so it
    // lives in its own device buffer and is rebuilt (and sent) only when that key changes
    std::vector<int> key; key.reserve(2 * K + D + 2);
    key.push_back(K); key.push_back(P.pn); key.insert(key.end(), as_i.begin(), as_i.end()); key.insert(key.end(), as_j.begin(), as_j.end()); key.insert(key.end(), pinv.begin(), pinv.end());
    int cs = -1;
    for (int q = 0; q < 4; ++q) if (c->chtabs[q].d() && c->chtabs[q].key == key) cs = q;
    const bool ct_hit = cs >= 0;
    if (!ct_hit) { cs = 0; for (int q = 1; q < 4; ++q) if (c->chtabs[q].used < c->chtabs[cs].used) cs = q; }      // (least recently used)
    vil_ctx::ChTab& ct = c->chtabs[cs];
    ct.used = ++c->chtab_clock; c->chtab_cur = cs;
    if (!ct_hit) {
        const int NPs = vd::chain_slab_nps(K), pn = P.pn;
        const int o_dg = 0, o_sub = vd::even_up(45 * K), o_pbc = o_sub + vd::even_up(81 * K), o_pp = o_pbc + 162 * K, o_rhs = o_pp + CHAIN_NPC_MAX * NPs;
        std::vector<int> tab, pq(9 * K, -1);
        int npc = 0;
        for (int jc = 0; jc < 9 * K; ++jc) if (pn > 0 && pinv[NV + jc] >= 0) pq[jc] = npc++;
        if (npc > CHAIN_NPC_MAX) pre_ok = false;       // (cannot happen: the prior's speed-bias blocks are neighbours -- checked for the chain path)
        auto ip = [&](int f, int la, int lb) { return f < 0 ? -1 : f * 931 + la * 30 + lb; };
        auto pr = [&](int r, int col) { if (pn <= 0) return -1; const int pi = pinv[r], pj = pinv[col]; return (pi >= 0 && pj >= 0) ? pi * pn + pj : -1; };
        // (IMU sources carry two indices: (index into the 931-double records + 1) in the low half, (index into the compact records of a one-launch iteration + 1) in the high half; 0: none)
        auto both = [&](int a) { if (a < 0) return 0; const int f = a / 931, ce = chain_rec_index(a % 931); return (a + 1) | ((f * VIL_CHAIN_REC + ce + 1) << 16); };
        auto emit = [&](int dst, int a, int b, int cc) { if (a < 0 && b < 0 && cc == -1) return; tab.push_back(dst); tab.push_back(both(a)); tab.push_back(both(b)); tab.push_back(cc); };
        for (int k = 0; k < K && pre_ok; ++k) {
            const int fi = as_i[k], fj = as_j[k];
            for (int i = 0; i < 9; ++i) for (int j = 0; j <= i; ++j) emit(o_dg + 45 * k + i * (i + 1) / 2 + j, ip(fi, 6 + i, 6 + j), ip(fj, 21 + i, 21 + j), pr(NV + 9 * k + i, NV + 9 * k + j));
            if (k + 1 < K) for (int q = 0; q < 9; ++q) for (int cc = 0; cc < 9; ++cc) emit(o_sub + 81 * k + q * 9 + cc, ip(fi, 21 + q, 6 + cc), -1, pr(NV + 9 * (k + 1) + q, NV + 9 * k + cc));
            for (int cc = 0; cc < 9; ++cc) {
                const int pj = pn > 0 ? pinv[NV + 9 * k + cc] : -1;
                emit(o_rhs + 9 * k + cc, fi < 0 ? -1 : fi * 931 + 900 + 6 + cc, fj < 0 ? -1 : fj * 931 + 900 + 21 + cc, pj >= 0 ? -pj - 2 : -1);
                for (int d = 0; d < 3; ++d) {              // pose rows of frames k-1, k, k+1: the IMU factors' share, compact
                    const int fr = k - 1 + d;
                    if (fr < 0 || fr >= K) continue;
                    for (int lr = 0; lr < 6; ++lr) {
                        const int a = (fi >= 0 && (fr == k || fr == k + 1)) ? ip(fi, fr == k ? lr : 15 + lr, 6 + cc) : -1;
                        const int b = (fj >= 0 && (fr == k - 1 || fr == k)) ? ip(fj, fr == k - 1 ? lr : 15 + lr, 21 + cc) : -1;
                        emit(o_pbc + ((k * 3 + d) * 6 + lr) * 9 + cc, a, b, -1);
                    }
                }
                if (pq[9 * k + cc] >= 0) for (int r = 0; r < NV; ++r) emit(o_pp + pq[9 * k + cc] * NPs + r, -1, -1, pr(r, NV + 9 * k + cc));      // the prior's share: every row
            }
        }
        {   // the chain workgroup deals consecutive entries to consecutive threads and every entry has its own target: sorted by source address, a wave's loads of
            // the IMU records (and of the prior) fall into a few cache lines each instead of one line per lane -- the gather is bound by the lines its loads touch
            const size_t ne = tab.size() / 4;
            std::vector<std::array<int, 4>> ent(ne);
            memcpy(ent.data(), tab.data(), 16 * ne);
            auto skey = [](const std::array<int, 4>& e) -> long long { return e[1] > 0 ? (e[1] >> 16) : e[2] > 0 ? (e[2] >> 16) : (1LL << 40) + (e[3] >= 0 ? (1LL << 32) + e[3] : -e[3]); };
            std::stable_sort(ent.begin(), ent.end(), [&](const std::array<int, 4>& x, const std::array<int, 4>& y) { return skey(x) < skey(y); });
            memcpy(tab.data(), ent.data(), 16 * ne);
        }
        tab.insert(tab.end(), pq.begin(), pq.end());       // behind the table: the chain column -> prior column map
        while (tab.size() & 3) tab.push_back(0);
        const size_t bytes = 4 * tab.size();
        // the previous table's DMA has left the pinned copy; a larger pair once the stream is idle (nobody reads the old one)
        { const int st = ct.st.begin(c->stream, bytes, 2 * bytes); if (st != VIL_OK) return st; }
        memcpy(ct.st.h.p, tab.data(), bytes);
        { const int st = ct.st.send(c->stream, bytes); if (st != VIL_OK) return st; }
        ct.n = ((int)tab.size() - ((9 * K + 3) & ~3)) / 4; ct.key.swap(key);
        built = true;
    }
    P.n_chtab = ct.n;
    if (ct.n > VIL_CHC_MAX) pre_ok = false;
    return VIL_OK;
}
// device allocation + single H2D copy: every slot of the image, the pointers that are not the arena's, the system sets; the parameter block goes to c->P
static int commit(vil_ctx* c, ImageBuilder& im, DevP& P, bool pre_ok, const vil_device_lidar* dl, const vil_problem* gp, const WinSrc* ws, size_t ar_cam) {
    Arena& ar = c->ar;
    if (im.oom) return VIL_ERR_DEVICE;
    const size_t tables = (ar.hsize + 255) & ~size_t(255), total = tables + ((ar.ssize + 255) & ~size_t(255));
    HIPCHK(ar.d.reserve(total, total + total / 4));
    for (const ImageBuilder::Fix& f : im.fix) *f.slot = ar.d.p + (f.scratch ? tables : 0) + f.off;
    if (dl) { P.pl_c = dl->plane_soa; P.pl_stride = dl->plane_stride; P.ed_c = dl->edge_soa; P.ed_stride = dl->edge_stride; }
    if (!gp) { P.glm_start = P.lm_start; P.glm_acol = P.lm_acol; P.gfcol = P.fcol; }
    if (pre_ok) { const vil_ctx::ChTab& ct = c->chtabs[c->chtab_cur]; P.chtab = ct.d(); P.chpq = ct.d() + 4 * (size_t)ct.n; }
    if (c->lidar_resident) c->lidar.tables(P);
    if (ws && P.pn) { P.px0 = ws->px0; P.pJ0 = ws->pJ0; P.pr0 = ws->pr0; P.pH = ws->pH; P.pg0 = ws->pg0; P.pc0 = ws->pc0; }      // the device prior slot, contractions included
    const size_t Lp = (size_t)std::max(P.L, 1), D = P.D;
    for (int q = 0; q < 2; ++q) {
        SysBuf& sb = P.sys[q];
        sb.S = sb.ar; sb.gred = sb.S + (size_t)D * D; sb.bc = sb.gred + D; sb.diag = sb.bc + D; sb.cost = sb.diag + D;
        sb.hll = sb.ar + ar_cam; sb.bl = sb.hll + Lp; sb.invp = sb.bl + Lp; sb.sl = sb.invp + Lp; sb.eA = sb.sl + Lp; sb.eO = sb.eA + 13 * Lp;
    }
    if (ar.hsize) {
        HIPCHK(hipMemcpyAsync(ar.d.p, ar.h.p, ar.hsize, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c->up_sent.record(c->stream));
    }
    if (ar.ssize) HIPCHK(hipMemsetAsync(ar.d.p + tables, 0, ar.ssize, c->stream));
    P.drop_role = -1; P.drop_launch = -1;
    c->P = P; c->K = P.K; c->L = P.L; c->D = P.D; c->NS = P.NS;
    c->mirror_state = false;
    if (!c->no_poll) { const int ms = ensure_mirror(c, (size_t)P.NS); if (ms != VIL_OK) return ms; }
    c->P.hctl = c->d_hctl; c->P.hseq = c->d_hseq; c->P.hstate = c->d_hstate;
    c->P.xorig = c->d_x0; c->P.gauge_on = c->gauge_on ? 1 : 0; c->P.setup_stat = c->d_status.p;
    return VIL_OK;
}
// what vil_marginalize_resident will need (a few passes over int tables; LiDAR points of pose 0 of a resident window: upload_lidar, from the unsliced slab counts)
static void marg_meta(vil_ctx* c, const vil_problem* p, const vil_problem* gp, const WinSrc* ws, const vil_device_lidar* dl) {
    vil_ctx::MargMeta& mm = c->mm;
    if (gp) p = gp;                                    // which blocks the collected factors touch is a property of the WHOLE window, the same on every rank
    mm.has_prior = p->prior.n > 0; mm.prior_kind.clear(); mm.prior_index.clear();
    if (mm.has_prior) { mm.prior_kind.assign(p->prior.blk_kind, p->prior.blk_kind + p->prior.nblk); mm.prior_index.assign(p->prior.blk_index, p->prior.blk_index + p->prior.nblk); }
    mm.obs0.assign(c->K, 0); mm.n_lm0 = 0; mm.imu01 = false; mm.use_td = p->use_td != 0;
    if (ws) {
        for (int l = 0; l < c->L; ++l) if (ws->lm_startf[l] == 0) { ++mm.n_lm0; for (int q = 1; q < ws->lm_nobs[l]; ++q) mm.obs0[q] = 1; }
        for (int f = 0; f < p->n_imu; ++f) if (p->imu_i[f] == 0 && p->imu_j[f] == 1 && ws->sum_dt[ws->islot[1]] < 10.0) mm.imu01 = true;
    } else {
        int last_l = -1;
        for (int f = 0; f < p->n_vis; ++f) if (p->vis_i[f] == 0) { mm.obs0[p->vis_j[f]] = 1; if (p->vis_l[f] != last_l) { ++mm.n_lm0; last_l = p->vis_l[f]; } }
        for (int f = 0; f < p->n_imu; ++f) if (p->imu_i[f] == 0 && p->imu_j[f] == 1 && p->imu_const[(size_t)f * 287 + 16] < 10.0) mm.imu01 = true;
    }
    mm.icp_ids.assign(p->icp_ids, p->icp_ids + 4 * (size_t)p->n_icp); mm.lps_ids.assign(p->lps_ids, p->lps_ids + 2 * (size_t)p->n_lps);
    if (!c->lidar_resident && !dl) {
        for (int f = 0; f < p->n_plane && !mm.lidar0; ++f) if (p->plane_pose[f] == 0) mm.lidar0 = true;
        for (int f = 0; f < p->n_edge && !mm.lidar0; ++f) if (p->edge_pose[f] == 0) mm.lidar0 = true;
    }
}
// ---- THE launch structure of the uploaded window, into c->ls and the fields of c->P that carry it: the kernels of an iteration, their grids and dynamic LDS
//      (granted here), the co-residency checks (probed here).  Every launch, the ladder of vil_solve_resident and vil_solve_batch read c->ls.
static int choose_structure(vil_ctx* c, const vil_problem* p, bool pre_ok) {
    DevP& P = c->P;
    Structure& S = c->ls;
    S = Structure();
    const int K = P.K, D = P.D, NV = P.NV;
    // (LiDAR workgroups can make several passes of two chunks -- fewer, longer workgroups when a window has more sweep roles than the device has compute units.
    //  Measured at configs[2], 496 sweep roles: 1 pass 1068 us per 13-iteration solve, 2 passes 1085, 4 passes 1120, 8 passes 1282: the dispatcher's second round
    //  balances better than any static packing.  One pass; the knob stays in the tuning build.)
    int R = 1;
    if (const char* ev = VIL_TUNE_ENV("VIL_LIDAR_REP")) R = std::max(1, atoi(ev));
    P.lidar_rep = R;
    const int per = VIL_SWEEP_THREADS / 256;
    S.n_sweep = P.n_imu + P.n_vwg + (P.n_pchunk + per * R - 1) / (per * R) + (P.n_echunk + per * R - 1) / (per * R) + 2;
    // visual workgroups: the staged factors, the landmark records, the dense operand rows of the largest chunk
    S.lds_sweep = sizeof(double) * (size_t)(VIS_LDS_FIXED + c->vis_gm);
    if (S.lds_sweep < 8 * 2048) S.lds_sweep = 8 * 2048;
    if (S.lds_sweep > 160 * 1024) return VIL_ERR_UNSUPPORTED;
    S.sweep_fn = P.vis_ts == 5 ? (const void*)k_sweep<5> : (const void*)k_sweep<2>;
    HIPCHK(grant_lds(c, S.sweep_fn, S.lds_sweep));
    S.n_reduce = gather_blocks(D, NV, RED_EPW, false);
    // ---- step kernel variant: the speed-bias part of the reduced matrix is a chain whenever every IMU factor couples (k, k+1)
    //      and the prior's speed-bias blocks are neighbours (VINS: exactly one) -> vil_chain.hpp; anything else: dense path
    bool chain = VIL_TUNE_ENV("VIL_DENSE_STEP") == nullptr;
    for (int f = 0; f < p->n_imu && chain; ++f) if (std::abs(p->imu_i[f] - p->imu_j[f]) > 1) chain = false;
    if (P.pn) {
        std::vector<int> psb;
        for (int b = 0; b < p->prior.nblk; ++b) if (p->prior.blk_kind[b] == VIL_BLK_SPEEDBIAS) psb.push_back(p->prior.blk_index[b]);
        for (int a : psb) for (int b : psb) if (std::abs(a - b) > 1) chain = false;
    }
    S.chain_rs = vd::chain_rs(K);
    const size_t Tp = (size_t)(NV + 1 + 15) / 16, tiles = (size_t)TILE_SZ * (Tp * (Tp + 1) / 2);
    const int Tw = (int)(Tp * (Tp + 1) / 2);
    if (chain) {
        const size_t wt = (size_t)vd::chain_wcols(K) * S.chain_rs, scr = vd::chain_scratch_doubles(K);
        const size_t fixed = step_static_lds((const void*)k_step<true, 1>) + 256;      // (the kernel's whole static LDS: StepShared + the gather / tile roles' scratch)
        if (8 * (tiles + wt + scr) + fixed <= 160 * 1024) { S.chain = 1; S.lds_step = 8 * (tiles + wt + scr); }
        else if (8 * (tiles + scr) + fixed <= 160 * 1024) { S.chain = 2; S.lds_step = 8 * (tiles + scr); }
    }
    // one GPU, chain windows: gather + step in ONE launch with the chain eliminated beside the gather (prechain 1, vil_prechain.hpp).
    // Until round 4 only up to K = 12: with ~100 kB of dynamic LDS per workgroup the ~1500 gather workgroups of a K = 20 window needed six rounds
    // on 256 compute units.  Windows the launch cannot hold (capacity check below) keep the separate gather and eliminate the chain inside
    // k_sweep, behind the IMU / prior workgroups' flags, with the W W^T tiles on extra workgroups of k_reduce (prechain 2).
    const size_t lds3 = 8 * (tiles + 54 * (size_t)K + 82 * (size_t)K + vd::even_up(9 * K) + 16), ldsc = 8 * vd::prechain_lds_doubles(K);
    const bool can_pre = !c->split && pre_ok && S.chain != 0 && Tp * (Tp + 1) / 2 <= 64 && lds3 + step_static_lds((const void*)k_step<true, 3>) + 256 <= 160 * 1024 && ldsc <= 150 * 1024;
    // (round 4: every window size -- the gather of a prechain solve forms the visual sub-space only, 551 workgroups at K = 20 instead of 1500)
    int kmerge = 20;
    if (const char* ev = VIL_TUNE_ENV("VIL_MERGE_K")) kmerge = atoi(ev);
    bool merged = can_pre && (c->launch_mode == 0 || c->launch_mode == 3 || c->launch_mode == 4) && K <= kmerge && std::max(lds3, ldsc) + step_static_lds((const void*)k_step<true, 3>) + 256 <= 160 * 1024 && VIL_TUNE_ENV("VIL_NO_MERGE") == nullptr;
    // the merged launch holds workgroups that spin on flags (master, helpers, one per W W^T tile) next to the finite ones they wait for (chain,
    // gather: lower block indices, dispatched first).  It is only taken when the device can hold every spinning workgroup AND one more at the
    // same time -- otherwise the waiters could occupy every slot before the last gather workgroup has found one (vil_coop.hpp)
    if (merged && !fits_per_xcd(1 + P.n_help + Tw + 1, coop_capacity(c, (const void*)k_step<true, 3>, std::max(lds3, ldsc)))) merged = false;
    S.prechain = merged ? 1 : (can_pre ? 2 : 0);
    if (S.prechain) {
        S.chain = 3;
        S.n_ww = Tw;
        if (merged) S.lds_step = std::max(lds3, ldsc);       // (the chain workgroup is one of the merged launch's)
        else {
            S.lds_step = lds3;
            S.lds_sweep = std::max(S.lds_sweep, ldsc);      // the chain workgroup rides in k_sweep
            HIPCHK(grant_lds(c, S.sweep_fn, S.lds_sweep));
            S.n_sweep += 1;
        }
    }
    // (the merged launch gathers 64 entries per 512-thread workgroup: half as many workgroups as the gather kernel's)
    const bool g64 = VIL_TUNE_ENV("VIL_GATHER32") == nullptr;
    S.n_gather_m = g64 ? gather_blocks(D, NV, 64, true) : gather_blocks(D, NV, RED_EPW, true);
    S.n_reduce_po = gather_blocks(D, NV, RED_EPW, true);
    S.rs_merged = merged ? (g64 ? 2 : 1) : 0; S.n_gather = merged ? S.n_gather_m : 0;
    // ---- the whole iteration in ONE launch (k_iter, vil_iter.hpp): whenever the merged gather + step launch is taken, the kernel's single dynamic-LDS size
    //      (the larger of the sweep roles' and the step roles' needs -- StepShared and the gather / tile scratch are carved from it) fits a compute unit, and
    //      the device holds the workgroups that wait for one another (master, helpers, tiles) at once.  vil_debug_set_launch_mode(3) keeps the two launches.
    if (merged && g64 && (c->launch_mode == 0 || c->launch_mode == 4) && S.n_sweep <= VIL_SFLAG_MAX && VIL_TUNE_ENV("VIL_NO_FUSE") == nullptr) {
        const size_t scratch = 8 * (size_t)(2 * VIS_TAB + 2 * 8 * (VIL_STEP_THREADS / 8) + 160);      // gather role: descriptor table | part[2][512] | index tables | red
        const size_t step_need = 8 * (size_t)VIL_SS_DOUBLES + std::max(std::max(lds3, ldsc), scratch);
        const size_t li = std::max(S.lds_sweep, step_need);
        const void* fn = P.vis_ts == 5 ? (const void*)k_iter<5> : (const void*)k_iter<2>;
        if (li <= 160 * 1024) {
            HIPCHK(grant_lds(c, fn, li));
            const int cap = coop_capacity(c, fn, li);
            if (fits_per_xcd(1 + P.n_help + Tw + 1, cap)) { S.fused = true; S.iter_fn = fn; S.lds_iter = li; S.n_sw = S.n_sweep; S.cap_fused = cap; }      // (+ the chain workgroup)
            // ---- the whole SOLVE in one resident launch (k_solve): the grid [sweep roles | chain | master | helpers | tiles] must fit the device at once with two
            //      workgroups to spare, and every gather item must find a workgroup that takes it as a duty (tiles, helpers, sweep roles): configs[1]-sized
            //      windows.  Everything else keeps one launch per iteration.  vil_debug_set_launch_mode(4) keeps k_iter.
            if (S.fused && c->launch_mode == 0 && VIL_TUNE_ENV("VIL_NO_PERSIST") == nullptr) {
                const size_t sweep_need = 8 * (size_t)(VIL_LC_DOUBLES + VIL_XL_DOUBLES) + std::max(S.lds_sweep, 8 * (size_t)2048 + scratch);      // [Ctl copy | state copy | role arrays (IMU roles: gather scratch behind them)]
                const size_t ls = std::max(sweep_need, step_need);
                const void* fs = vil_k_solve_fn(P.vis_ts);
                if (ls <= 160 * 1024 && K <= 15) {
                    HIPCHK(grant_lds(c, fs, ls));
                    const int grid = S.n_sweep + 2 + P.n_help + Tw, n_cap = S.n_sweep + P.n_help + Tw;
                    if (fits_per_xcd(grid, coop_capacity(c, fs, ls)) && S.n_gather_m <= n_cap) { S.persist = true; S.lds_solve = ls; }
                }
            }
        }
    }
    P.chain = S.chain; P.chain_rs = S.chain_rs; P.prechain = S.prechain; P.rs_merged = S.rs_merged; P.n_ww = S.n_ww; P.n_gather = S.n_gather; P.n_sw = S.n_sw;
    static const void* const chain_step[4] = {nullptr, (const void*)k_step<true, 1>, (const void*)k_step<true, 2>, (const void*)k_step<true, 3>};
    S.step_fn = chain_step[S.chain];
    if (!S.chain) {
        const size_t T = (size_t)(D + 1 + 15) / 16;
        S.lds_step = 8 * TILE_SZ * (T * (T + 1) / 2);      // 16x16-tiled (row stride 17) lower storage incl. the rhs row
        S.step_fn = (const void*)k_step<true, 0>;
        if (S.lds_step + step_static_lds(S.step_fn) + 256 > 160 * 1024) {
            S.lds_step = 8 * (size_t)TILE_SZ * T;      // tile array in global memory; LDS stages the active tile column of the factorisation (T tiles)
            S.step_fn = (const void*)k_step<false, 0>;
            if (S.lds_step + step_static_lds(S.step_fn) + 256 > 160 * 1024) return VIL_ERR_UNSUPPORTED;
        }
    }
    HIPCHK(grant_lds(c, S.step_fn, S.lds_step));
    return VIL_OK;
}
// one-time set-up: IMU sqrt-information, prior contraction
static int upload_setup(vil_ctx* c, const WinSrc* ws, bool check_setup, const int* wd_track, const int* wd_startf) {
    const DevP& P = c->P;
    if (!ws) HIPCHK(hipMemsetAsync(c->d_status.p, 0, sizeof(int), c->stream));      // (resident window: nothing writes it -- its status word is the window's own, vil_win_solve -- and a 4-byte fill is a 5 us launch)
    if (ws) {
        // resident window: expand the landmark table into the factor tables, gather the IMU records, copy the state -- everything k_setup
        // would compute (sqrt-information, prior contractions) already sits next to its source
        WinPack W; memset(&W, 0, sizeof W);
        W.L = P.L; W.F = P.n_vis; W.stride = P.vis_stride; W.T = ws->T;
        W.lm_start = P.lm_start; W.lm_track = wd_track; W.lm_startf = wd_startf; W.store = ws->store;
        for (int k = 0; k < P.K; ++k) { W.fslot[k] = ws->fslot[k]; W.islot[k] = ws->islot[k]; }
        W.vis_c = const_cast<double*>(P.vis_c); W.vis_i = const_cast<int*>(P.vis_i); W.vis_j = const_cast<int*>(P.vis_j); W.vis_l = const_cast<int*>(P.vis_l); W.fcol = const_cast<int*>(P.fcol); W.vfinv = P.vfinv;
        W.n_imu = P.n_imu; W.rec = ws->d_rec; W.U = ws->d_U; W.imu_c = const_cast<double*>(P.imu_c); W.imu_U = const_cast<double*>(P.imu_U);
        W.NS = P.NS; W.x0 = P.x[0]; W.x1 = P.x[1]; W.xorig = c->d_x0;
        const int nbf = (P.n_vis + 255) / 256, nbs = (P.NS + 255) / 256;
        hipLaunchKernelGGL(k_win_pack, dim3(nbf + P.n_imu + nbs), dim3(256), 0, c->stream, W, nbf);
    }
    const int nb_setup = ws ? 0 : P.n_imu + (P.pn ? 64 : 0);
    if (nb_setup > 0) hipLaunchKernelGGL(k_setup, dim3(nb_setup), dim3(VIL_THREADS), 0, c->stream, P, const_cast<double*>(P.imu_U), c->d_status.p);
    if (check_setup) {
        c->h_word.p[0] = 0;
        HIPCHK(hipMemcpyAsync(c->h_word.p, c->d_status.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipGetLastError());
        if (c->h_word.p[0] != 0) return VIL_ERR_NOT_POSITIVE_DEFINITE;
    }
    return VIL_OK;
}

// check_setup: wait for k_setup's verdict (an IMU covariance that is not positive definite) and return it; false: nothing is waited for --
// the first step kernel of the solve ends it with that status (DevP::setup_stat), and the launches of the solve queue up behind the upload
static int upload_impl(vil_ctx* c, const vil_problem* p, const vil_state* s, bool sharded, const vil_device_lidar* dl = nullptr, const vil_problem* gp = nullptr, int vis_f0 = 0, bool check_setup = true, const WinSrc* ws = nullptr) {
    if (!c) return VIL_ERR_INVALID_ARGUMENT;
    int st = validate(p, s, dl != nullptr, ws != nullptr);
    if (st != VIL_OK) return st;                 // an invalid problem leaves the resident one untouched
    c->invalidate();                             // from here on the arena is rewritten: resident only again after a complete upload
    c->reset_pending = false;
    HIPCHK(hipSetDevice(c->device));
#ifdef VIL_TUNING
    static const bool up_trace = getenv("VIL_UPLOAD_TRACE") != nullptr;
    auto up_t0 = std::chrono::steady_clock::now();
    #define UPTICK(name) do { if (up_trace) { const auto t_ = std::chrono::steady_clock::now(); fprintf(stderr, "[upload] %-10s %7.1f us\n", name, std::chrono::duration<double, std::micro>(t_ - up_t0).count()); up_t0 = t_; } } while (0)
#else
    #define UPTICK(name) do {} while (0)
#endif
    HIPCHK(c->up_sent.wait());
    c->ar.reset();
    ImageBuilder im{c->ar};
    DevP P; memset(&P, 0, sizeof P);
    upload_state(c, im, p, s, ws, P);
    UPTICK("head");
    int* wd_track = nullptr; int* wd_startf = nullptr;       // device copies of the landmark table (resident window)
    if ((st = upload_visual(c, im, p, ws, gp, vis_f0, P, &wd_track, &wd_startf)) != VIL_OK) return st;
    UPTICK("visual");
    if ((st = upload_lidar(c, im, p, dl, P)) != VIL_OK) return st;
    UPTICK("lidar");
    std::vector<int> pinv;
    if ((st = upload_imu_prior(c, im, p, ws, P, pinv)) != VIL_OK) return st;
    UPTICK("imu+prior");
    const size_t ar_cam = upload_workspace(c, im, ws, gp, sharded, P);
    UPTICK("ws-puts");
    bool pre_ok = false, built = false;
    if ((st = chain_table(c, p, sharded, P, pinv, pre_ok, built)) != VIL_OK) return st;
    if (built) UPTICK("chtab-new");
    if (const char* ev = VIL_TUNE_ENV("VIL_SKIP")) P.skip_mask = atoi(ev);
    P.n_help = vil_helpers_for(P.L, c->device);
    UPTICK("workspace");
    if ((st = commit(c, im, P, pre_ok, dl, gp, ws, ar_cam)) != VIL_OK) return st;
    marg_meta(c, p, gp, ws, dl);
    if ((st = choose_structure(c, p, pre_ok)) != VIL_OK) return st;
    UPTICK("h2d+attrs");
    if ((st = upload_setup(c, ws, check_setup, wd_track, wd_startf)) != VIL_OK) return st;
    UPTICK("setup");
    c->uploaded = true; c->resident_kind = 2;    // vil_upload / vil_solve promote it to 1
    return VIL_OK;
}

// rank r keeps the visual factors of its landmark range, a contiguous slice of the LiDAR points, and
// (rank 0 only) the IMU / prior / ICP / LPS factors.  Landmark indices and the state stay global.
static int upload_sharded(vil_ctx* c, const vil_problem* p, const vil_state* s) {
    Comm& cm = c->comm;
    int st = validate(p, s);                     // the factor prefix indexes with vis_l: check the tables first
    if (st != VIL_OK) return cm.agree(c->stream, st);  // every rank sees the same problem, but stay collective anyway
    std::vector<int> lms(p->L + 1, 0);           // factor prefix per landmark (factors sorted by landmark): the rule of vil_shard_ranges
    for (int f = 0; f < p->n_vis; ++f) lms[p->vis_l[f] + 1]++;
    for (int l = 0; l < p->L; ++l) lms[l + 1] += lms[l];
    cm.set_owners(lms, p->L, p->K);
    const int f0 = lms[shard_cut(lms, p->L, cm.rank, cm.world)], f1 = lms[shard_cut(lms, p->L, cm.rank + 1, cm.world)];
    vil_problem q = *p;
    q.n_vis = f1 - f0; q.vis_i = p->vis_i + f0; q.vis_j = p->vis_j + f0; q.vis_l = p->vis_l + f0; q.vis_const = p->vis_const + (size_t)f0 * 14;
    if (p->n_plane == VIL_LIDAR_RESIDENT && p->n_edge == VIL_LIDAR_RESIDENT) { /* the slabs of this context already hold this rank's slice of every frame (vil_lidar_push) */ }
    else {
        const int eb = (int)((long long)p->n_edge * cm.rank / cm.world), ee = (int)((long long)p->n_edge * (cm.rank + 1) / cm.world);
        const int pb = (int)((long long)p->n_plane * cm.rank / cm.world), pe = (int)((long long)p->n_plane * (cm.rank + 1) / cm.world);
        q.n_edge = ee - eb; q.edge_pose = p->edge_pose + eb; q.edge_const = p->edge_const + (size_t)eb * 9;
        q.n_plane = pe - pb; q.plane_pose = p->plane_pose + pb; q.plane_const = p->plane_const + (size_t)pb * 7;
    }
    if (cm.rank != 0) { q.n_imu = 0; q.n_icp = 0; q.n_lps = 0; q.prior.n = 0; q.prior.nblk = 0; }
    st = cm.agree(c->stream, upload_impl(c, &q, s, true, nullptr, p, f0));       // e.g. rank 0's IMU set-up failed: every rank reports it
    if (st != VIL_OK) c->uploaded = false;
    return st;
}

static int upload_window(vil_ctx* c, const vil_problem* p, const vil_state* s, bool check_setup) {
    if (!c) return VIL_ERR_INVALID_ARGUMENT;
    if (c->comm.world > 1 && !c->comm.ready()) return VIL_ERR_COMM;             // vil_comm_ipc_export without vil_comm_ipc_init
    const int st = (c->comm.sharded()) ? upload_sharded(c, p, s)      // a world > 1 context without a communicator works un-sharded
                                                           : upload_impl(c, p, s, false, nullptr, nullptr, 0, check_setup);
    if (st == VIL_OK) c->resident_kind = 1;
    return st;
}
int vil_upload(vil_ctx* c, const vil_problem* p, const vil_state* s) { return upload_window(c, p, s, true); }

// Multi-GPU: ONE collective per trust-region iteration.  Every rank sweeps its shard into set 0 -- the reduced camera
// system of its factors plus the landmark arrays (h_ll, b_l, 1/pivot, scale, e_l) of the landmarks it owns, zeros elsewhere -- the
// whole set is all-reduced into set 1, and every rank runs the complete single-GPU step kernel (helper workgroups, chain path)
// on identical data: identical decisions, identical candidates, no second exchange.  view 0: what the sweep / gather write
// (both buffer slots alias set 0: the partial system is consumed by the collective at once); view 1: what the step kernel reads.
static DevP view(const vil_ctx* c, int which) {
    DevP P = c->P;
    if (c->split) { P.sys[0] = P.sys[1] = c->P.sys[which]; if (which == 1) { P.rank = 0; P.world = 1; } }
    return P;
}
// launches of the kernels choose_structure picked (k_sweep, k_iter, k_step take (DevP, SolveOpts))
static void launch_chosen(vil_ctx* c, const void* fn, unsigned grid, unsigned threads, size_t lds, DevP P, SolveOpts so) {
    void* args[] = {&P, &so};
    hipLaunchKernel(fn, dim3(grid), dim3(threads), args, lds, c->stream);
}
static int launch_sweep(vil_ctx* c, const SolveOpts& so) {
    launch_chosen(c, c->ls.sweep_fn, c->ls.n_sweep, VIL_SWEEP_THREADS, c->ls.lds_sweep, view(c, 0), so);
    return VIL_OK;
}
// one trust-region iteration as ONE launch (vil_iter.hpp); only un-sharded solves of a window the upload marked `fused`
static int launch_iter(vil_ctx* c, const SolveOpts& so) {
    DevP Pi = c->P;
    Pi.gather_pose_only = 1;
    Pi.prof = c->profiling ? c->d_prof.p : nullptr; Pi.wg_launch = c->profiling ? c->wg_launch : -1;
    launch_chosen(c, c->ls.iter_fn, c->ls.n_sweep + 1 + c->ls.n_gather_m + 1 + c->P.n_help + c->ls.n_ww, VIL_STEP_THREADS, c->ls.lds_iter, Pi, so);      // [sweep roles | chain | master | helpers | W W^T tiles | gather]
    return VIL_OK;
}
// the whole solve as ONE resident launch (vil_iter.hpp, k_solve); budget_ticks: what is left of max_time_s on the device's 100 MHz clock (0: no cap)
static int launch_solve(vil_ctx* c, const SolveOpts& so, long long budget_ticks) {
    DevP Pi = c->P;
    Pi.gather_pose_only = 1; Pi.prof = c->stamps ? c->d_prof.p : nullptr; Pi.wg_launch = -1; Pi.persist = 1;
    vil_k_solve_launch(c->P.vis_ts, (unsigned)(c->ls.n_sweep + 2 + c->P.n_help + c->ls.n_ww), c->ls.lds_solve, c->stream, Pi, so, budget_ticks);      // [sweep roles | chain | master | helpers | W W^T tiles]
    return VIL_OK;
}
static int launch_reduce_step(vil_ctx* c, const SolveOpts& so, bool step, hipEvent_t ev_mid = nullptr, hipEvent_t ev_coll = nullptr) {
    const Structure& S = c->ls;
    const bool merged = step && S.rs_merged;          // one GPU: the gather rides in the step kernel's launch (vil_step.hpp)
    // (chain eliminated inside k_sweep: one workgroup per W W^T tile rides in the gather launch, one for the inverses of the chain's diagonal blocks in the step launch;
    //  a solve on the prechain path reads S' on the visual sub-space + the diagonal only -- vil_linearize, the marginalisation and sharded solves all of it)
    if (!merged) {
        DevP Pg = view(c, 0);
        const bool po = step && S.prechain != 0 && !c->split;
        Pg.gather_pose_only = po ? 1 : 0;
        const int ng = po ? S.n_reduce_po : S.n_reduce;
        hipLaunchKernelGGL(k_reduce, dim3(ng + ((step && S.prechain == 2) ? S.n_ww : 0)), dim3(VIL_THREADS), 0, c->stream, Pg, ng);
    }
    if (ev_mid) hipEventRecord(ev_mid, c->stream);
    if (c->split) {                                    // the one collective of the iteration
        const int st = c->comm.sum(c->stream, c->P.sys[0].ar, c->P.sys[1].ar, c->span, c->D, true, c->span);      // (S' first: its lower triangle travels; landmark arrays: the owners' slices)
        if (st != VIL_OK) return st;
    }
    if (ev_coll) hipEventRecord(ev_coll, c->stream);
    if (!step) return VIL_OK;
    DevP Ps = view(c, 1);
    if (!merged) { Ps.rs_merged = 0; Ps.n_ww = 0; Ps.n_gather = 0; }
    Ps.gather_pose_only = merged ? 1 : 0;
    const int g = 1 + c->P.n_help + (merged ? (S.prechain ? 1 : 0) + S.n_ww + S.n_gather_m : (S.prechain == 2 ? 1 : 0));      // (prechain 2: + prechain_inverses)
    launch_chosen(c, S.step_fn, g, VIL_STEP_THREADS, S.lds_step, Ps, so);
    return VIL_OK;
}

// vil_reset_state is deferred: whoever touches the resident state next restores it first (a solve inside its init launch)
static void flush_reset(vil_ctx* c) {
    if (!c->reset_pending) return;
    hipLaunchKernelGGL(k_state_reset, dim3((c->NS + 255) / 256), dim3(256), 0, c->stream, c->P.x[0], c->P.x[1], (const double*)c->d_x0, c->NS);
    c->reset_pending = false;
}
static int init_ctl(vil_ctx* c, const vil_options* o, int lin_mode) {
    // (a kernel with the values in its arguments: an asynchronous copy out of the one pinned h_ctl could be overtaken by the next call's init --
    //  vil_win_marginalize / push / drop return without a stream synchronisation)
    static_assert(sizeof(Ctl) % 8 == 0, "Ctl is cleared as doubles");
    if (c->reset_pending && lin_mode == 0) {               // vil_reset_state + vil_solve_resident: the state copy rides in the init launch
        hipLaunchKernelGGL(k_solve_init_reset, dim3((c->NS + 255) / 256), dim3(256), 0, c->stream, c->P.ctl, ++c->solve_gen, o->initial_radius, o->min_mu, lin_mode, c->P.x[0], c->P.x[1], (const double*)c->d_x0, c->NS, c->P.abortf, c->d_xsave);
        c->reset_pending = false;
    } else {
        flush_reset(c);
        double* const xs = lin_mode == 0 ? c->d_xsave : nullptr;      // (a solve keeps its start state aside: vil_solve_resident's retry / failure path)
        hipLaunchKernelGGL(k_solve_init, dim3(xs ? (c->NS + 255) / 256 : 1), dim3(256), 0, c->stream, c->P.ctl, ++c->solve_gen, o->initial_radius, o->min_mu, lin_mode, c->P.abortf, (const double*)c->P.x[0], xs, c->NS);
    }
    memset(c->h_ctl.p, 0, sizeof(Ctl));
    return VIL_OK;
}

int vil_profile_enable(vil_ctx* c, int on) {
    if (!c) return VIL_ERR_INVALID_ARGUMENT;
    HIPCHK(hipSetDevice(c->device));
    if (on && c->ev.empty()) { c->ev.resize(2 * VIL_MAX_CHUNK + 2); for (auto& e : c->ev) HIPCHK(hipEventCreate(&e)); c->ev_mid.resize(VIL_MAX_CHUNK + 1); for (auto& e : c->ev_mid) HIPCHK(hipEventCreate(&e)); c->ev_coll.resize(VIL_MAX_CHUNK + 1); for (auto& e : c->ev_coll) HIPCHK(hipEventCreate(&e)); }
    if (on && !c->d_prof.p) { HIPCHK(c->d_prof.reserve(64 * VIL_PROF_SLOTS + 2 * VIL_PROF_WGS, 64 * VIL_PROF_SLOTS + 2 * VIL_PROF_WGS)); HIPCHK(hipMemset(c->d_prof.p, 0, 8 * (64 * VIL_PROF_SLOTS + 2 * VIL_PROF_WGS))); }
    c->profiling = on == 1;
    c->stamps = on == 2;          // 2: the phase stamps alone -- the launch structure stays the library's choice (the persistent solve keeps its one launch; no events)
    return VIL_OK;
}
int vil_profile_read(vil_ctx* c, vil_profile* out, int reset) {
    if (!c || !out) return VIL_ERR_INVALID_ARGUMENT;
    *out = c->prof;
    if (reset) c->prof = vil_profile{0, 0.0, 0, 0.0, 0.0, 0.0};
    return VIL_OK;
}

int vil_reset_state(vil_ctx* c) {
    if (!c || !c->uploaded) return VIL_ERR_INVALID_ARGUMENT;
    HIPCHK(hipSetDevice(c->device));
    c->reset_pending = true;                                 // (carried out by the next call that touches the state: flush_reset / init_ctl)
    c->mirror_state = false;
    return VIL_OK;
}

// The best rung of the ladder of launch structures: 0 the whole solve in one resident launch (k_solve), 1 one launch per iteration (k_iter), 2 sweep + gather / step launches
static int top_rung(const vil_ctx* c) {
    return !c->ls.fused || c->split ? 2 : (c->ls.persist && !c->profiling ? 0 : 1);
}

// ---- one attempt at a solve, stage by stage: solve_attempt (below them) reads top to bottom ----------------------------------------------------
// What an attempt runs, by value: the options and their device form, the start of the solve on the host clock, the rung of the ladder (top_rung), no graph replay
struct Attempt {
    vil_options o; SolveOpts so; std::chrono::steady_clock::time_point t0; int rung; bool direct;
    bool persist() const { return rung == 0; }
    bool fused() const { return rung <= 1; }
    double elapsed_s() const { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
};
// iterations are enqueued in chunks without host round trips; the first chunk is sized by the previous solve of
// this context (consecutive windows of a tracker need similar iteration counts), later chunks are short
static int first_chunk(const vil_ctx* c, bool fused) {
    int chunk = std::min(15, std::max(3, c->last_live));
    // One-launch iterations write the result out themselves as soon as a launch finds the solve finished (vil_iter.hpp): a chunk that is too LONG costs the stream
    // ~5 us per dead launch and the host nothing, one that is too SHORT costs a host round trip (~70 us) and a second chunk.  The first solve of an upload -- what a
    // tracker runs per image, iteration counts wandering by one or two from image to image -- therefore enqueues the largest count of the last eight solves plus two;
    // re-solves of one upload (graph replay, the same count again and again) keep the exact size.
    if (fused && c->solves_since_upload == 0) { int mx = 3; for (int v : c->recent_live) mx = std::max(mx, v); chunk = std::min(VIL_MAX_CHUNK, mx + 2); }
    if (c->profiling) chunk = std::min(chunk, (int)c->ev.size() / 2 - 1);      // (events bracket every launch of a chunk: ev[2 q], ev[2 q + 1], ev[2 launched])
    return chunk;
}
// Repeated solves of ONE upload (bench, re-solves after a rejected frame) replay a captured hipGraph of the chunk:
// ~2 % less inter-kernel gap.  The first solve of an upload launches directly -- capturing costs more than it saves.
// hipGraph replay: un-sharded solves, and sharded ones whose collective is the library's own kernels (peer-buffer exchange).  RCCL calls are
// launched directly (whether a given RCCL build captures correctly is not something this path bets the multi-GPU run on); the in-process
// communicator synchronises on the host.  Polling the finished solve's mirror works for everything that is in stream order.
static bool may_replay(vil_ctx* c, const Attempt& a) {
    if (c->use_graph < 0) { const char* ev = VIL_TUNE_ENV("VIL_GRAPH"); c->use_graph = ev ? atoi(ev) : 1; }
    const bool no_graph = c->split && !c->comm.capturable();
    return c->use_graph && c->solves_since_upload > 0 && !c->profiling && !no_graph && !a.direct && !a.persist();      // (direct: a retry, or a solve with a debug hook in its parameter block)
}
// The hipGraph of a chunk of n iterations and its k_finish: the cached one of this (n, options), or a fresh capture.  *exec == nullptr: launch directly
static int chunk_graph(vil_ctx* c, const Attempt& a, int n, hipGraphExec_t* exec) {
    *exec = nullptr;
    if (c->graph_failed) return VIL_OK;
    for (auto& g : c->graphs) if (g.n == n && memcmp(&g.so, &a.so, sizeof a.so) == 0) *exec = g.exec;
    if (*exec) return VIL_OK;
    hipGraph_t graph = nullptr;
    HIPCHK(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
    int cst = VIL_OK;
    for (int q = 0; q < n && cst == VIL_OK; ++q) { if (a.fused()) cst = launch_iter(c, a.so); else { launch_sweep(c, a.so); cst = launch_reduce_step(c, a.so, true, nullptr); } }
    hipLaunchKernelGGL(k_finish, dim3(1), dim3(VIL_SWEEP_THREADS), 0, c->stream, view(c, 0), -1);
    const hipError_t ce = hipStreamEndCapture(c->stream, &graph);
    const bool forced = c->fail_capture > 0;
    if (forced) --c->fail_capture;
    if (cst != VIL_OK || ce != hipSuccess || forced || hipGraphInstantiate(exec, graph, nullptr, nullptr, 0) != hipSuccess) {
        // a chunk that cannot be captured or instantiated (a collective the RCCL build at hand does not capture, a driver out of graph memory): nothing has
        // run yet, so THIS solve and every later one of the context take the direct launches (enqueue_chunk) -- the caller (optimization()) has no retry
        (void)hipGetLastError();
        if (graph) hipGraphDestroy(graph);
        *exec = nullptr; c->graph_failed = true;
        // (a capture that could not be ENDED may leave the stream in an invalidated capture state: the direct launches would fail the same way.
        //  The collectives advance no host-side state while captured -- the peer-buffer exchange counts in device memory, when its kernels run)
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (ce != hipSuccess && (hipStreamIsCapturing(c->stream, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone)) { (void)hipGetLastError(); return VIL_ERR_DEVICE; }
    } else {
        hipGraphDestroy(graph);
        c->graphs.push_back({n, a.so, *exec});
    }
    return VIL_OK;
}
// The three ways a pass puts iterations on the stream.  Each returns how many (> 0), or a status (< 0).
static int enqueue_replay(vil_ctx* c, hipGraphExec_t exec, int n) {
    HIPCHK(hipGraphLaunch(exec, c->stream));
    return n;
}
static int enqueue_resident(vil_ctx* c, const Attempt& a, int left) {
    // ONE launch runs every iteration and writes the result out; the time cap travels with it (the master reads the device clock where ceres reads its own)
    long long ticks = 0;
    if (a.o.max_time_s > 0) ticks = std::max(1LL, (long long)((a.o.max_time_s - a.elapsed_s()) * 1e8));
    if (c->stamps && !c->ev.empty()) HIPCHK(hipEventRecord(c->ev[0], c->stream));
    const int st = launch_solve(c, a.so, ticks);
    if (st != VIL_OK) return st;
    if (c->stamps && !c->ev.empty()) HIPCHK(hipEventRecord(c->ev[1], c->stream));
    return left;      // every iteration the solve has left
}
static int enqueue_chunk(vil_ctx* c, const Attempt& a, int n) {
    for (int q = 0; q < n; ++q) {
        if (c->profiling) HIPCHK(hipEventRecord(c->ev[2 * q], c->stream));
        if (a.fused()) {
            // (one launch: the events bracket the whole iteration; what the sweep roles took inside it comes from the launch's own clock stamps: account_stamps)
            const int st = launch_iter(c, a.so);
            if (st != VIL_OK) return st;
            continue;
        }
        launch_sweep(c, a.so);
        if (c->profiling) HIPCHK(hipEventRecord(c->ev[2 * q + 1], c->stream));
        const int st = launch_reduce_step(c, a.so, true, c->profiling ? c->ev_mid[q] : nullptr, c->profiling ? c->ev_coll[q] : nullptr);
        if (st != VIL_OK) return st;          // a failed collective fails on every rank (Comm::sum): nobody is left waiting
    }
    if (c->profiling) HIPCHK(hipEventRecord(c->ev[2 * n], c->stream));
    hipLaunchKernelGGL(k_finish, dim3(1), dim3(VIL_SWEEP_THREADS), 0, c->stream, view(c, 0), -1);      // the write-out of a solve that ended in the chunk's last iteration
    return n;
}
// solve_finish leaves Ctl, the final state and then the solve generation in pinned host memory: poll that word instead of
// synchronising (the no-op tail of the chunk is not waited for, nothing is copied afterwards).  A chunk that runs out without
// finishing is seen by hipStreamQuery and takes the copy + synchronise route, as do profiling and multi-rank solves.
// Leaves *c->h_ctl.p filled; *via_mirror is set when it came through the mirror.
static int await_result(vil_ctx* c, bool* via_mirror) {
    bool polled = false;
    if (c->d_hseq && !c->profiling && !(c->split && c->comm.host_synchronised())) {
        volatile int* seq = (volatile int*)(c->h_mirror.h + sizeof(Ctl));
        const int gen = c->solve_gen;
        const auto tp0 = std::chrono::steady_clock::now();
        for (long spin = 1;; ++spin) {
            if (*seq == gen) { polled = true; break; }
            if ((spin & 0x3ff) == 0) {
                const hipError_t q = hipStreamQuery(c->stream);
                if (q == hipSuccess) { polled = *seq == gen; break; }
                if (q != hipErrorNotReady) return VIL_ERR_DEVICE;
                if (std::chrono::steady_clock::now() - tp0 > std::chrono::seconds(2)) break;
            }
        }
        if (polled) { std::atomic_thread_fence(std::memory_order_acquire); memcpy(c->h_ctl.p, c->h_mirror.h, sizeof(Ctl)); *via_mirror = true; }
    }
    if (!polled) {
        HIPCHK(hipMemcpyAsync(c->h_ctl.p, c->P.ctl, sizeof(Ctl), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    return VIL_OK;
}
// profiling: the HIP events of a chunk of `launched` direct launches, for those of them that found the solve unfinished
static int account_events(vil_ctx* c, bool fused, int launched, int sweeps_before) {
    int live = c->h_ctl.p->n_sweeps - sweeps_before;   // launches that found done == 0
    live = std::max(0, std::min(live, launched));
    for (int q = 0; q < live; ++q) {
        float ms = 0.f;
        if (fused) {      // one launch: the events give its whole duration (to step_ms; the sweep phase's share moves to sweep_ms from the launch's own stamps: account_stamps)
            HIPCHK(hipEventElapsedTime(&ms, c->ev[2 * q], c->ev[2 * q + 2])); c->prof.step_ms += ms; c->prof.sweep_launches++; c->prof.step_launches++;
            continue;
        }
        HIPCHK(hipEventElapsedTime(&ms, c->ev[2 * q], c->ev[2 * q + 1])); c->prof.sweep_ms += ms; c->prof.sweep_launches++;
        HIPCHK(hipEventElapsedTime(&ms, c->ev[2 * q + 1], c->ev[2 * q + 2])); c->prof.step_ms += ms; c->prof.step_launches++;
        HIPCHK(hipEventElapsedTime(&ms, c->ev[2 * q + 1], c->ev_mid[q])); c->prof.reduce_ms += ms;
        HIPCHK(hipEventElapsedTime(&ms, c->ev_mid[q], c->ev_coll[q])); c->prof.collective_ms += ms;
    }
    return VIL_OK;
}
// (sharded solves ignore the host-timed cap: the ranks' clocks disagree, and a rank that stops enqueuing chunks leaves its peers waiting in
//  the collective of the next iteration -- the iteration cap is the bound every rank applies identically)
static bool host_cap_reached(const vil_ctx* c, const Attempt& a) {
    return !c->split && a.o.max_time_s > 0 && a.elapsed_s() >= a.o.max_time_s;
}
// ceres max_solver_time_in_seconds (estimator.cpp:1411): the host ends the solve; the accepted state is written out on request
static int finish_at_cap(vil_ctx* c) {
    hipLaunchKernelGGL(k_finish, dim3(1), dim3(VIL_SWEEP_THREADS), 0, c->stream, c->P, (int)VIL_TERM_MAX_TIME);
    HIPCHK(hipMemcpyAsync(c->h_ctl.p, c->P.ctl, sizeof(Ctl), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return VIL_OK;
}
// the launches' own clock stamps (100 MHz): the sweep phase of a one-launch iteration = first workgroup started -> last sweep role posted
static int account_stamps(vil_ctx* c, bool persist, int n_sweeps) {
    std::vector<unsigned long long>& hp = c->last_stamps; hp.assign((size_t)64 * VIL_PROF_SLOTS, 0ull);
    HIPCHK(hipMemcpyAsync(hp.data(), c->d_prof.p, 8 * hp.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (persist && c->stamps && !c->ev.empty()) {      // the resident launch as a whole (HIP events on the library's stream): step_ms / step_launches; its iterations: sweep_launches
        float ms = 0.f;
        HIPCHK(hipEventSynchronize(c->ev[1]));
        HIPCHK(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
        c->prof.step_ms += ms; c->prof.step_launches++; c->prof.sweep_launches += n_sweeps;
    }
    for (int q = 0; q < n_sweeps; ++q) {
        const unsigned long long* r = hp.data() + (size_t)q * VIL_PROF_SLOTS;
        if (!r[0] || !r[1]) continue;
        const unsigned long long t0 = ~r[0];
        // the phase table describes a FULL iteration (linearisation, dense solve, step): the last launch of a solve judges a candidate and ends -- averaged in,
        // as until round 5, it pulled every late stamp ~10 % towards zero ("master done 50.3 us" was 55.7)
        if (r[10] >= t0 && r[12] >= t0) {
            for (int k = 1; k < VIL_PROF_SLOTS; ++k) if (r[k] >= t0) c->phase_us[k] += (double)(r[k] - t0) * 0.01;
            c->phase_n++;
            if (q + 1 < n_sweeps && r[VIL_PROF_SLOTS]) { c->phase_us[0] += (double)(~r[VIL_PROF_SLOTS] - t0) * 0.01; c->period_n++; }      // (persistent solve: first role of this iteration -> first role of the next)
        }
        const double sweep_us = (double)(r[1] - t0) * 0.01, gather_us = r[5] > r[1] ? (double)(r[5] - r[1]) * 0.01 : 0.0;
        c->prof.sweep_ms += sweep_us * 1e-3; c->prof.step_ms -= sweep_us * 1e-3; c->prof.reduce_ms += gather_us * 1e-3;      // (the events gave the whole launch to step_ms)
    }
    return VIL_OK;
}
// Ctl -> vil_summary, the history that sizes the next solve's first chunk, and the status of the attempt
static int summarize(vil_ctx* c, const Attempt& a, bool via_mirror, vil_summary* sum) {
    const Ctl& ctl = *c->h_ctl.p;
    c->solves_since_upload++;
    c->last_live = ctl.n_sweeps;
    c->recent_live[c->recent_at++ & 7] = ctl.n_sweeps;
    memset(sum, 0, sizeof *sum);
    sum->iterations = ctl.iter; sum->successful_steps = ctl.nsucc; sum->termination = ctl.term;
    sum->initial_cost = ctl.initial_cost; sum->final_cost = ctl.cost_cur;
    for (int i = 0; i < VIL_MAX_TRACE; ++i) { sum->cost_trace[i] = ctl.cost_trace[i]; sum->radius_trace[i] = ctl.radius_trace[i]; }
    sum->t_solve_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a.t0).count();
    // (the accepted state is x[0] = x[1] on the device, gauge-fixed when asked for: solve_finish ran in stream order; whoever reads the
    //  window afterwards orders itself behind it on the stream)
    c->mirror_state = via_mirror && c->d_hstate != nullptr;
    if (ctl.status != 0) return ctl.status;
    if (!std::isfinite(ctl.cost_cur)) return VIL_ERR_NON_FINITE;
    return VIL_OK;
}
// One attempt at the solve on rung `rung` of the ladder (top_rung).
// *gave_up: a wait inside a launch gave up (status -2 from the master, or no launch ever reported `done`): the caller decides about the retry.
static int solve_attempt(vil_ctx* c, const vil_options* o, vil_summary* sum, const std::chrono::steady_clock::time_point t0, const bool direct, const int rung, bool* gave_up) {
    const Attempt a = {*o, to_dev_opts(o), t0, rung, direct};
    c->mirror_state = false;
    *gave_up = false;
    int st = init_ctl(c, o, 0);
    if (st != VIL_OK) return st;
    const bool stamped = (c->profiling || (c->stamps && a.persist())) && a.fused() && c->d_prof.p != nullptr;      // the launches leave their own clock stamps in d_prof
    if (stamped) HIPCHK(hipMemsetAsync(c->d_prof.p, 0, 8 * 64 * VIL_PROF_SLOTS, c->stream));
    // every iteration = sweep + gather + step kernel; `done` turns the tail of a chunk into no-ops, and the first sweep launch that finds
    // the solve finished writes the result out (vil_finish.hpp); k_finish at the end of every chunk covers a solve that ends in its last iteration
    bool finished = false, via_mirror = false;
    int chunk = first_chunk(c, a.fused());
    for (int it = 0; it <= o->max_iterations + 8 && !finished; chunk = 3) {
        const int sweeps_before = (it == 0) ? 0 : c->h_ctl.p->n_sweeps;
        const int left = o->max_iterations + 9 - it, nthis = std::min(chunk, left);
        hipGraphExec_t exec = nullptr;
        if (may_replay(c, a)) { st = chunk_graph(c, a, nthis, &exec); if (st != VIL_OK) return st; }
        int n;      // iterations this pass puts on the stream (< 0: a status)
        if (exec) n = enqueue_replay(c, exec, nthis);
        else if (a.persist()) n = enqueue_resident(c, a, left);
        else n = enqueue_chunk(c, a, nthis);
        if (n < 0) return n;
        it += n;
        st = await_result(c, &via_mirror);
        if (st != VIL_OK) return st;
        finished = c->h_ctl.p->done != 0;
        if (c->profiling) { st = account_events(c, a.fused(), n, sweeps_before); if (st != VIL_OK) return st; }
        if (!finished && host_cap_reached(c, a)) { st = finish_at_cap(c); if (st != VIL_OK) return st; finished = true; via_mirror = false; }
    }
    HIPCHK(hipGetLastError());
    // a wait inside a launch gave up (vil_math.hpp, spin_until_eq): the master ended the solve with status -2 -- or never ran, and the launches drained without a `done`
    if (!finished || c->h_ctl.p->status == VIL_ERR_DEVICE) { *gave_up = true; return VIL_ERR_DEVICE; }
    if (stamped && c->h_ctl.p->n_sweeps <= 64) { st = account_stamps(c, a.persist(), c->h_ctl.p->n_sweeps); if (st != VIL_OK) return st; }
    return summarize(c, a, via_mirror, sum);
}

int vil_solve_resident(vil_ctx* c, const vil_options* o, vil_summary* sum) {
    if (!c || !o || !sum || !c->uploaded || c->resident_kind != 1) return VIL_ERR_INVALID_ARGUMENT;   // vil_marginalize / vil_eval_factors / vil_linearize replaced the window
    if (o->precision != 0 && o->precision != 1) return VIL_ERR_UNSUPPORTED;
    HIPCHK(hipSetDevice(c->device));
    const auto t0 = std::chrono::steady_clock::now();
    // the step kernel's master, helpers and (merged launch) tile workgroups wait for one another inside a launch: like the other persistent kernels of
    // the library a solve holds its device's gate until its result has arrived, so that it never shares the device with a half-resident
    // k_pose_solve / k_vgicp_align of another thread (vil_coop.hpp).  Not taken by the ranks of a communicator (in-process, peer buffers, RCCL): they wait
    // for EACH OTHER's launches inside the per-iteration collective -- two ranks driven from threads of one process would deadlock on it.
    // (the solves of a vil_solve_batch share the gate: one launch per iteration each, never the persistent solve -- the batch has checked that their waiting workgroups fit together)
    std::unique_lock<std::shared_mutex> coop_lock(vilcoop::gate(c->device), std::defer_lock);
    std::shared_lock<std::shared_mutex> coop_shared(vilcoop::gate(c->device), std::defer_lock);
    if (!c->split) { if (c->in_batch) coop_shared.lock(); else coop_lock.lock(); }
    if ((c->P.gauge_on != 0) != c->gauge_on) {            // vil_set_gauge_fix since the upload: the captured graphs carry the old flag
        c->P.gauge_on = c->gauge_on ? 1 : 0;
        for (auto& g : c->graphs) hipGraphExecDestroy(g.exec);
        c->graphs.clear();
    }
    // vil_debug_drop_flag: armed for THIS solve only (its launches carry the hook in their parameter block -- launched directly, the captured graphs do not know it)
    const bool hook = c->drop_role != -1;
    const bool hook_sticky = hook && (c->drop_launch & 0x10000) != 0;      // (... and for the retry as well: the test of a solve that fails on both structures)
    c->P.drop_role = c->drop_role; c->P.drop_launch = c->drop_launch & 0xffff;
    c->drop_role = -1; c->drop_launch = -1;
    // The ladder of launch structures: the persistent solve (EVERY role resident at once), one launch per iteration (the handful of waiting workgroups resident at
    // once), two launches per iteration.  A wait inside a launch that gives up (vil_math.hpp: 50 ms of the device clock) moves the SAME solve one rung down, from the
    // state it started from -- co-residency is a property of the whole device (another process's persistent kernel, a CU mask the occupancy query does not see) and the
    // library's gate is process-local, so this is the way out instead of a hang; the caller (optimization(), estimator.cpp:1400-1414) has no retry of its own.
    // A rung that gives up in two consecutive solves is left out for the next 256 solves of the context (a masked device must not pay the wait per image).
    auto restore = [&]() -> int {
        HIPCHK(hipStreamSynchronize(c->stream));      // the drained launches of the attempt (every wait returns at once behind the abort word)
        hipLaunchKernelGGL(k_state_reset, dim3((c->NS + 255) / 256), dim3(256), 0, c->stream, c->P.x[0], c->P.x[1], (const double*)c->d_xsave, c->NS);
        c->reset_pending = false; c->mirror_state = false;
        return VIL_OK;
    };
    for (int q = 0; q < 2; ++q) if (c->rung_cooldown[q] > 0) c->rung_cooldown[q]--;
    int first = top_rung(c);
    if (first == 0 && (c->in_batch || c->rung_cooldown[0] > 0)) first = 1;      // (the solves of a batch share the device: never the resident launch)
    if (first == 1 && c->rung_cooldown[1] > 0) first = 2;
    bool gave_up = false, retried = false;
    int st = VIL_ERR_DEVICE;
    for (int rung = first; rung <= 2; ++rung) {
        st = solve_attempt(c, o, sum, t0, hook || retried, rung, &gave_up);
        if (!hook_sticky) { c->P.drop_role = -1; c->P.drop_launch = -1; }
        if (!gave_up) {
            if (rung < 2) c->rung_fail_run[rung] = 0;
            if (retried) c->n_recovered++;
            c->P.drop_role = -1; c->P.drop_launch = -1;
            return st;
        }
        if (rung < 2 && ++c->rung_fail_run[rung] >= 2) { c->rung_cooldown[rung] = 256; c->rung_fail_run[rung] = 0; }
        const int rs = restore();
        if (rs != VIL_OK) return rs;
        retried = true;
    }
    c->P.drop_role = -1; c->P.drop_launch = -1;
    c->n_aborted++;
    HIPCHK(hipStreamSynchronize(c->stream));
    return VIL_ERR_DEVICE;                             // the resident state is the one the solve started from
}

// B windows solved CONCURRENTLY on one device: every context on its own stream, one launch per trust-region iteration each (k_iter), driven by a host thread per
// context.  A single window leaves most of the device idle behind its sweep phase (one master workgroup on dependent fp64 chains); B of them interleave -- the
// single-GPU form of the `replicas` leg of a multi-GPU run.  Each window's result is bit-equal to its solo solve with one launch per iteration.
int vil_solve_batch(vil_ctx** ctxs, int32_t n, const vil_options* o, vil_summary* sums, int32_t* statuses) {
    if (!ctxs || n < 1 || n > 16 || !o || !sums || !statuses) return VIL_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < n; ++i) {
        if (!ctxs[i] || !ctxs[i]->uploaded || ctxs[i]->resident_kind != 1 || ctxs[i]->split || ctxs[i]->device != ctxs[0]->device) return VIL_ERR_INVALID_ARGUMENT;
        for (int j = 0; j < i; ++j) if (ctxs[j] == ctxs[i]) return VIL_ERR_INVALID_ARGUMENT;
    }
    // how many of them may wait inside their launches at once: the waiting workgroups of all (master, helpers, tiles, chain) must fit the device per XCD
    int group = n;
    {
        int waiting = 0, cap = 1 << 30;
        for (int i = 0; i < n; ++i) { const vil_ctx* c = ctxs[i]; waiting = std::max(waiting, 2 + c->P.n_help + c->ls.n_ww); if (c->ls.fused && c->ls.cap_fused > 0) cap = std::min(cap, c->ls.cap_fused); }
        while (group > 1 && !fits_per_xcd(group * waiting, cap)) --group;
        // ... and at most half of the device may wait: the workgroups the waiting ones wait for need the other half.  How many launches really run at once is the
        // runtime's number of hardware queues (four unless GPU_MAX_HW_QUEUES says otherwise): with eight queues eight windows of configs[1] waited on 208 of 256
        // compute units and the batch took 14 ms instead of 2 (profiles/r06_concurrent_windows_8queues.json, before this rule)
        {
            const char* qe = getenv("GPU_MAX_HW_QUEUES");
            const int hwq = qe && atoi(qe) > 0 ? atoi(qe) : 4;
            while (group > 1 && std::min(group, hwq) * waiting > cap / 2) --group;
        }
    }
    for (int i0 = 0; i0 < n; i0 += group) {
        const int m = std::min(group, n - i0);
        std::vector<std::thread> th;
        for (int k = 0; k < m; ++k) {
            vil_ctx* c = ctxs[i0 + k];
            th.emplace_back([c, o, sums, statuses, i0, k]() { c->in_batch = true; statuses[i0 + k] = vil_solve_resident(c, o, &sums[i0 + k]); c->in_batch = false; });
        }
        for (auto& t : th) t.join();
    }
    for (int i = 0; i < n; ++i) if (statuses[i] != VIL_OK) return statuses[i];
    return VIL_OK;
}

int vil_recovery_counts(vil_ctx* c, int64_t* recovered, int64_t* failed) {
    if (!c) return VIL_ERR_INVALID_ARGUMENT;
    if (recovered) *recovered = c->n_recovered;
    if (failed) *failed = c->n_aborted;
    return VIL_OK;
}

int vil_download_state(vil_ctx* c, vil_state* s) {
    if (!c || !s || !c->uploaded || s->K != c->K || s->L != c->L) return VIL_ERR_INVALID_ARGUMENT;
    HIPCHK(hipSetDevice(c->device));
    flush_reset(c);
    const double* x = nullptr;
    std::vector<double> xb;
    if (c->mirror_state) x = (const double*)(c->h_mirror.h + sizeof(Ctl) + 64);      // left there by solve_finish: no device operation
    else {
        xb.resize(c->NS);
        HIPCHK(hipMemcpyAsync(xb.data(), c->P.x[0], 8 * (size_t)c->NS, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        x = xb.data();
    }
    for (int i = 0; i < c->NS; ++i) if (!std::isfinite(x[i])) return VIL_ERR_NON_FINITE;
    const int K = c->K, L = c->L;
    memcpy(s->pose, &x[0], 8 * (size_t)7 * K); memcpy(s->speedbias, &x[7 * K], 8 * (size_t)9 * K);
    memcpy(s->ex_pose, &x[16 * K], 56); s->td[0] = x[16 * K + 7];
    if (L) memcpy(s->inv_depth, &x[16 * K + 8], 8 * (size_t)L);
    return VIL_OK;
}

int vil_solve(vil_ctx* c, const vil_problem* p, vil_state* s, const vil_options* o, vil_summary* sum) {
    if (!c || !p || !s || !o || !sum) return VIL_ERR_INVALID_ARGUMENT;
    const auto t0 = std::chrono::steady_clock::now();
    int st = upload_window(c, p, s, false);            // nothing is waited for: the solve's launches queue up behind the upload
    if (st != VIL_OK) return st;
    const auto t1 = std::chrono::steady_clock::now();
    st = vil_solve_resident(c, o, sum);
    sum->t_prepare_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
    if (st != VIL_OK) return st;                       // state left unchanged on any error
    const auto t2 = std::chrono::steady_clock::now();
    st = vil_download_state(c, s);
    sum->t_readback_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t2).count();
    return st;
}

int vil_solve_device_lidar(vil_ctx* c, const vil_problem* p, const vil_device_lidar* dl, void* producer_stream, vil_state* s, const vil_options* o, vil_summary* sum) {
    if (!c || !p || !dl || !s || !o || !sum) return VIL_ERR_INVALID_ARGUMENT;
    if ((p->n_plane > 0 && (!dl->plane_soa || dl->plane_stride < p->n_plane)) || (p->n_edge > 0 && (!dl->edge_soa || dl->edge_stride < p->n_edge))) return VIL_ERR_INVALID_ARGUMENT;
    if (c->comm.sharded()) return VIL_ERR_UNSUPPORTED;
    const auto t0 = std::chrono::steady_clock::now();
    HIPCHK(hipSetDevice(c->device));
    if (producer_stream && (hipStream_t)producer_stream != c->stream) {      // the tables are written by work on another stream: order after it on the device
        HIPCHK(c->dep_ev.record((hipStream_t)producer_stream));
        HIPCHK(hipStreamWaitEvent(c->stream, c->dep_ev.ev, 0));
    }
    int st = upload_impl(c, p, s, false, dl);
    if (st != VIL_OK) return st;
    c->resident_kind = 1;
    const auto t1 = std::chrono::steady_clock::now();
    st = vil_solve_resident(c, o, sum);
    sum->t_prepare_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
    if (st != VIL_OK) return st;
    const auto t2 = std::chrono::steady_clock::now();
    st = vil_download_state(c, s);
    sum->t_readback_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t2).count();
    return st;
}

static hipError_t ensure_pin(vil_ctx* c, size_t bytes) { return c->h_pin.reserve((bytes + 7) / 8, (bytes + 7) / 8); }

int vil_eval_factors(vil_ctx* c, const vil_problem* p, const vil_state* s, int cls, double* r, double* J) {
    if (!c || !r) return VIL_ERR_INVALID_ARGUMENT;
    int st = upload_impl(c, p, s, false);
    if (st != VIL_OK) return st;
    const DevP& P = c->P;
    size_t nr = 0, nj = 0; int nfac = 0;
    switch (cls) {
        case VIL_FACTOR_IMU: nfac = P.n_imu; nr = 15; nj = 480; break;
        case VIL_FACTOR_VISUAL: nfac = P.n_vis; nr = 2; nj = 46; break;
        case VIL_FACTOR_ICP: nfac = P.n_icp; nr = 3; nj = 84; break;
        case VIL_FACTOR_LPS: nfac = P.n_lps; nr = 3; nj = 42; break;
        case VIL_FACTOR_EDGE: nfac = P.n_edge; nr = 3; nj = 21; break;
        case VIL_FACTOR_PLANE: nfac = P.n_plane; nr = 1; nj = 7; break;
        case VIL_FACTOR_PRIOR: nfac = P.pn ? 1 : 0; nr = P.pn; nj = 0; for (int b = 0; b < P.pnblk; ++b) nj += (size_t)P.pn * blk_doubles(p->prior.blk_kind[b]); break;
        default: return VIL_ERR_INVALID_ARGUMENT;
    }
    if (nfac == 0) return VIL_OK;
    const size_t br = 8 * nr * nfac, bj = J ? 8 * nj * nfac : 0;
    vilhost::Grown<char> t_r, t_J; vilhost::Grown<int> t_joff;      // (freed on every return)
    HIPCHK(t_r.reserve(br, br));
    if (J) HIPCHK(t_J.reserve(bj, bj));
    double* const d_r = (double*)t_r.p; double* const d_J = (double*)t_J.p;
    const double* x = P.x[0];
    const int nb = (nfac + VIL_THREADS - 1) / VIL_THREADS;
    switch (cls) {
        case VIL_FACTOR_IMU: hipLaunchKernelGGL(k_eval_imu, dim3(nfac), dim3(VIL_THREADS), 0, c->stream, P, x, d_r, d_J); break;
        case VIL_FACTOR_VISUAL: hipLaunchKernelGGL(k_eval_visual, dim3(nb), dim3(VIL_THREADS), 0, c->stream, P, x, d_r, d_J); break;
        case VIL_FACTOR_ICP: hipLaunchKernelGGL(k_eval_rel, dim3(2), dim3(VIL_THREADS), 0, c->stream, P, x, 1, d_r, d_J); break;
        case VIL_FACTOR_LPS: hipLaunchKernelGGL(k_eval_rel, dim3(2), dim3(VIL_THREADS), 0, c->stream, P, x, 0, d_r, d_J); break;
        case VIL_FACTOR_EDGE: hipLaunchKernelGGL(k_eval_lidar<3>, dim3(nb), dim3(VIL_THREADS), 0, c->stream, P, x, d_r, d_J); break;
        case VIL_FACTOR_PLANE: hipLaunchKernelGGL(k_eval_lidar<1>, dim3(nb), dim3(VIL_THREADS), 0, c->stream, P, x, d_r, d_J); break;
        case VIL_FACTOR_PRIOR:
            HIPCHK(t_joff.reserve(c->prior_joff.size(), c->prior_joff.size()));
            HIPCHK(hipMemcpyAsync(t_joff.p, c->prior_joff.data(), 4 * c->prior_joff.size(), hipMemcpyHostToDevice, c->stream));
            hipLaunchKernelGGL(k_eval_prior, dim3(1), dim3(VIL_THREADS), 8 * (size_t)P.pn, c->stream, P, x, d_r, d_J, t_joff.p);
            break;
    }
    HIPCHK(ensure_pin(c, br + bj));
    HIPCHK(hipMemcpyAsync(c->h_pin.p, d_r, br, hipMemcpyDeviceToHost, c->stream));
    if (J) HIPCHK(hipMemcpyAsync((char*)c->h_pin.p + br, d_J, bj, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipGetLastError());
    const double* hr = c->h_pin.p; const double* hj = (const double*)((char*)c->h_pin.p + br);
    if (cls == VIL_FACTOR_EDGE || cls == VIL_FACTOR_PLANE) {   // undo the pose sort
        const std::vector<int>& perm = cls == VIL_FACTOR_EDGE ? c->edge_perm : c->plane_perm;
        for (int sidx = 0; sidx < nfac; ++sidx) {
            const int f = perm[sidx];
            memcpy(r + (size_t)f * nr, hr + (size_t)sidx * nr, 8 * nr);
            if (J) memcpy(J + (size_t)f * nj, hj + (size_t)sidx * nj, 8 * nj);
        }
    } else { memcpy(r, hr, br); if (J) memcpy(J, hj, bj); }
    return VIL_OK;
}

int vil_eval_lidar_functors(vil_ctx* c, int32_t kind, int32_t n, const double* consts, const double* q_lb, const double* t_lb, const double* pose7, double* r, double* J) {
    if (!c || kind < VIL_LIDAR_EDGE || kind > VIL_LIDAR_DISTANCE || n < 0 || (n > 0 && !consts) || !q_lb || !t_lb || !pose7 || !r) return VIL_ERR_INVALID_ARGUMENT;
    if (n == 0) return VIL_OK;
    HIPCHK(hipSetDevice(c->device));
    const int nc = kind == VIL_LIDAR_EDGE ? 9 : (kind == VIL_LIDAR_PLANE3 ? 12 : (kind == VIL_LIDAR_PLANE_NORM ? 7 : 6)), nr = (kind == VIL_LIDAR_EDGE || kind == VIL_LIDAR_DISTANCE) ? 3 : 1;
    LidarFunctorArgs A;
    { double R[9]; quat_to_R_host(q_lb, R); for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) A.Rbl[3 * i + j] = R[3 * j + i];          // body <- LiDAR: (R_lb^T, -R_lb^T t_lb), as the window upload
      for (int i = 0; i < 3; ++i) A.tbl[i] = -(A.Rbl[3 * i] * t_lb[0] + A.Rbl[3 * i + 1] * t_lb[1] + A.Rbl[3 * i + 2] * t_lb[2]); }
    memcpy(A.pose, pose7, sizeof A.pose);
    const size_t bc = 8 * (size_t)nc * n, br = 8 * (size_t)nr * n, bj = J ? 8 * (size_t)nr * 7 * n : 0;
    vilhost::Grown<char> t_c, t_r, t_J;      // (freed on every return)
    HIPCHK(t_c.reserve(bc, bc)); HIPCHK(t_r.reserve(br, br));
    if (J) HIPCHK(t_J.reserve(bj, bj));
    double* const d_c = (double*)t_c.p; double* const d_r = (double*)t_r.p; double* const d_J = (double*)t_J.p;
    HIPCHK(hipMemcpyAsync(d_c, consts, bc, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_eval_lidar_functors, dim3((n + VIL_THREADS - 1) / VIL_THREADS), dim3(VIL_THREADS), 0, c->stream, (int)kind, (int)n, d_c, A, d_r, d_J);
    HIPCHK(hipMemcpyAsync(r, d_r, br, hipMemcpyDeviceToHost, c->stream));
    if (J) HIPCHK(hipMemcpyAsync(J, d_J, bj, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipGetLastError());
    return VIL_OK;
}

int vil_linearize(vil_ctx* c, const vil_problem* p, const vil_state* s, const vil_options* o, double* cost, double* S, double* g) {
    if (!c || !o || !cost || !S || !g) return VIL_ERR_INVALID_ARGUMENT;
    int st = vil_upload(c, p, s);
    if (st != VIL_OK) return st;
    const SolveOpts so = to_dev_opts(o);
    st = init_ctl(c, o, 1);
    if (st != VIL_OK) return st;
    launch_sweep(c, so);                                   // partial records of system set 1 (cand = 1 - cur)
    launch_reduce_step(c, so, false);
    const size_t D = c->D;
    HIPCHK(ensure_pin(c, 8 * (D * D + D + 1)));
    const double* src = c->P.sys[1].ar;        // un-sharded: the candidate set (cur = 0); sharded: the all-reduced set
    HIPCHK(hipMemcpyAsync(c->h_pin.p, src, 8 * D * D, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(c->h_pin.p + D * D, src + D * D, 8 * D, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(c->h_pin.p + D * D + D, src + D * D + 3 * D, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipGetLastError());
    memcpy(S, c->h_pin.p, 8 * D * D); memcpy(g, c->h_pin.p + D * D, 8 * D); *cost = c->h_pin.p[D * D + D];
    return VIL_OK;
}

// common tail of vil_marginalize / vil_marginalize_resident: the normal equations of the collected factors sit in sys[1] (or the
// all-reduce staging buffer); Schur complement + square root on the device (k_marg), block metadata with the address shift as an
// index remap (estimator.cpp:1599-1611, 1654-1677)
static int marg_finish(vil_ctx* c, const int K, const bool old_, const int drop_pose, const std::vector<char>& pose_t, const std::vector<char>& sb_t,
                       const bool ex_t, const bool td_t, const bool use_td, const int n_lm_elim, const vil_state* s, vil_prior_out* out,
                       const bool to_slot = false, vil_win_prior_info* winfo = nullptr) {
    int st = VIL_OK;
    // ---- which reduced columns are dropped / kept (canonical kept order: poses, speed-biases, ex, td) ----------------
    const int D = c->D;
    std::vector<int> drop_cols, keep_cols, kinds, index;
    if (pose_t[drop_pose]) for (int k = 0; k < 6; ++k) drop_cols.push_back(6 * drop_pose + k);
    if (old_ && sb_t[0]) for (int k = 0; k < 9; ++k) drop_cols.push_back(6 * K + 7 + k);
    for (int k = 0; k < K; ++k) if (pose_t[k] && k != drop_pose) { kinds.push_back(VIL_BLK_POSE); index.push_back(k); for (int q2 = 0; q2 < 6; ++q2) keep_cols.push_back(6 * k + q2); }
    for (int k = 0; k < K; ++k) if (sb_t[k] && !(old_ && k == 0)) { kinds.push_back(VIL_BLK_SPEEDBIAS); index.push_back(k); for (int q2 = 0; q2 < 9; ++q2) keep_cols.push_back(6 * K + 7 + 9 * k + q2); }
    if (ex_t) { kinds.push_back(VIL_BLK_EX); index.push_back(0); for (int q2 = 0; q2 < 6; ++q2) keep_cols.push_back(6 * K + q2); }
    if (td_t && use_td) { kinds.push_back(VIL_BLK_TD); index.push_back(0); keep_cols.push_back(6 * K + 6); }
    const int nd = (int)drop_cols.size(), n = (int)keep_cols.size();
    int n_max, nblk_max, x0_max;
    vil_prior_capacity(K, &n_max, &nblk_max, &x0_max);
    if (n > n_max || n > 136 || nd > 15 || (int)kinds.size() > nblk_max || n <= 0 || nd <= 0) return VIL_ERR_UNSUPPORTED;
    // ---- device work space + kernel ------------------------------------------------------------------------------
    const size_t nn = (size_t)n * n;
    const size_t bytes = 8 * ((size_t)nd * nd * 2 + nd + nn * 5 + (size_t)n * 3) + 4 * (size_t)(nd + n) + 8192 + 256;
    HIPCHK(c->marg_ws.reserve(bytes, bytes));      // grow-only work space: no allocation on the per-frame path once warm
    char* dw = c->marg_ws.p;
    size_t off = 0;
    auto take = [&](size_t b2) { char* r = dw + off; off += (b2 + 255) & ~size_t(255); return r; };
    MargDev M;
    M.D = D; M.nd = nd; M.n = n; M.eps = 1e-8;
    M.S = c->P.sys[1].S; M.g = M.S + (size_t)D * D;
    int* d_drop = (int*)take(4 * (size_t)(nd + n)); int* d_keep = d_drop + nd;       // one table, one copy
    M.drop_cols = d_drop; M.keep_cols = d_keep;
    M.Add = (double*)take(8 * (size_t)nd * nd); M.Vd = (double*)take(8 * (size_t)nd * nd); M.wd = (double*)take(8 * (size_t)nd);
    M.T = (double*)take(8 * nn);
    M.V = (double*)take(8 * nn); M.w = (double*)take(8 * (size_t)n);
    M.J0 = (double*)take(8 * (2 * nn + 2 * (size_t)n)); M.A = M.J0 + nn; M.r0 = M.A + nn; M.b = M.r0 + n;      // what goes back to the host: one block, one copy
    M.stat = (int*)take(32);
    M.ts = (unsigned long long*)take(8 * 16); c->d_marg_ts = M.ts;
    if (off > bytes) return VIL_ERR_DEVICE;
    // the column table travels through pinned memory: the copy is asynchronous and the resident window never waits for it (the next use
    // of this staging area is a whole solve away)
    HIPCHK(ensure_pin(c, 8 * (nn * 2 + 2 * (size_t)n + 16 * (size_t)K + 8) + 4 * (size_t)(nd + n) + 64));
    int* hcols = (int*)((char*)c->h_pin.p + 8 * (nn * 2 + 2 * (size_t)n + 16 * (size_t)K + 8));
    for (int q = 0; q < nd; ++q) hcols[q] = drop_cols[q];
    for (int q = 0; q < n; ++q) hcols[nd + q] = keep_cols[q];
    HIPCHK(hipMemcpyAsync(d_drop, hcols, 4 * (size_t)(nd + n), hipMemcpyHostToDevice, c->stream));
    {
        const size_t a_bytes = 8 * nn, cap = 156 * 1024;
        if (a_bytes > cap) return VIL_ERR_UNSUPPORTED;
        const size_t dyn = std::max<size_t>(4096, a_bytes);
        if (dyn > 48 * 1024) HIPCHK(grant_lds(c, (const void*)k_marg, dyn));
        hipLaunchKernelGGL(k_marg, dim3(1), dim3(MARG_THREADS), dyn, c->stream, M, 0);
        if (!VIL_TUNE_ENV("VIL_MARG_PIVOTED")) {               // un-pivoted factorisation on the matrix cores first; pivoted fallback below
            const size_t Tm = (size_t)(n + 1 + 15) / 16, tb = 8 * (size_t)TILE_SZ * (Tm * (Tm + 1) / 2);
            if (tb + sizeof(vd::StepShared) + 512 <= 160 * 1024) {
                if (tb > 48 * 1024) HIPCHK(grant_lds(c, (const void*)k_marg_fast, tb));
                hipLaunchKernelGGL(k_marg_fast, dim3(1), dim3(VIL_STEP_THREADS), tb, c->stream, M);
            }
        }
        hipLaunchKernelGGL(k_marg, dim3(1), dim3(MARG_THREADS), dyn, c->stream, M, 1);
    }
    if (to_slot) {
        // resident window: the new prior goes device-to-device into the other prior slot (J0, r0, x0 from the device state, contractions);
        // nothing is read back, nothing is waited for.  A non-finite result raises the window's status word.
        st = c->win.commit_prior(c->stream, K, old_, n, nd + n_lm_elim, (int)kinds.size(), kinds.data(), index.data(), nullptr, M.J0, M.r0, c->P.x[0]);
        if (st != VIL_OK) return st;
        if (winfo) {
            vil_prior pb; c->win.prior_blocks(pb);
            winfo->n = n; winfo->nblk = pb.nblk; winfo->m = nd + n_lm_elim;
            for (int b = 0; b < pb.nblk; ++b) { winfo->blk_kind[b] = pb.blk_kind[b]; winfo->blk_index[b] = pb.blk_index[b]; winfo->blk_col[b] = pb.blk_col[b]; }
        }
        return VIL_OK;
    }
    const size_t ncam = 16 * (size_t)K + 8;
    HIPCHK(hipMemcpyAsync(c->h_pin.p, M.J0, 8 * (2 * nn + 2 * (size_t)n), hipMemcpyDeviceToHost, c->stream));      // J0 | A | r0 | b
    // x0 of the new prior = the state the factors were LINEARISED at, i.e. the device state (the reference stores the very values it
    // marginalises at, marginalization_factor.cpp:110-139) -- not whatever the caller holds
    double* hx = c->h_pin.p + 2 * nn + 2 * (size_t)n;
    HIPCHK(hipMemcpyAsync(hx, c->P.x[0], 8 * ncam, hipMemcpyDeviceToHost, c->stream));
    int mstat[4] = {0, 0, 0, 0};
    if (VIL_TUNE_ENV("VIL_MARG_DEBUG")) HIPCHK(hipMemcpyAsync(mstat, M.stat, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipGetLastError());
    if (VIL_TUNE_ENV("VIL_MARG_DEBUG")) fprintf(stderr, "[vil_marginalize] n=%d nd=%d one-sided Jacobi stages: %d (dropped block) %d (n x n, %.1f sweeps)\n", n, nd, mstat[0], mstat[1], mstat[1] / (double)(((n + 1) & ~1) - 1));
    for (size_t e = 0; e < 2 * nn + 2 * (size_t)n; ++e) if (!std::isfinite(c->h_pin.p[e])) return VIL_ERR_NON_FINITE;
    // ---- getParameterBlocks with the address shift as an index remap (estimator.cpp:1599-1611, 1654-1677) --------------
    out->n = n; out->m = nd + n_lm_elim; out->nblk = (int)kinds.size();
    memcpy(out->J0, c->h_pin.p, 8 * nn); memcpy(out->r0, c->h_pin.p + 2 * nn, 8 * (size_t)n);
    if (out->A) memcpy(out->A, c->h_pin.p + nn, 8 * nn);
    if (out->b) memcpy(out->b, c->h_pin.p + 2 * nn + n, 8 * (size_t)n);
    int col = 0, xo = 0;
    for (size_t b = 0; b < kinds.size(); ++b) {
        const int kind = kinds[b], idx = index[b];
        out->blk_kind[b] = kind;
        out->blk_index[b] = blk_shift(kind, idx, old_, K); out->blk_col[b] = col;
        const double* src = kind == VIL_BLK_POSE ? hx + 7 * idx : (kind == VIL_BLK_SPEEDBIAS ? hx + 7 * K + 9 * idx : (kind == VIL_BLK_EX ? hx + 16 * K : hx + 16 * K + 7));
        const int gs = blk_doubles(kind), ls = blk_cols(kind);
        for (int k = 0; k < gs; ++k) out->x0[xo + k] = src[k];
        xo += gs; col += ls;
    }
    return VIL_OK;
}

int vil_marginalize(vil_ctx* c, const vil_problem* p, const vil_state* s, const vil_options* o, const vil_marg_spec* spec, vil_prior_out* out) {
    if (!c || !p || !s || !o || !spec || !out) return VIL_ERR_INVALID_ARGUMENT;
    { const int vst = validate(p, s); if (vst != VIL_OK) return vst; }      // the host tables are indexed below, before upload_impl sees them
    const int K = p->K;
    if (K < 3) return VIL_ERR_INVALID_ARGUMENT;
    const bool old_ = spec->flag == VIL_MARGIN_OLD;
    const int drop_pose = old_ ? 0 : K - 2;
    // ---- derived sub-problem: the factors MarginalizationInfo collects (estimator.cpp:1489-1589 / 1626-1641), every block free
    vil_problem q = *p;
    q.pose_const = nullptr; q.sb_const = nullptr; q.lm_const = nullptr; q.ex_const = 0; q.td_const = 0;
    q.n_edge = 0; q.n_plane = 0; q.edge_pose = nullptr; q.plane_pose = nullptr; q.edge_const = nullptr; q.plane_const = nullptr;
    std::vector<int> imu_i, imu_j, vis_i, vis_j, vis_l, icp_ids, lps_ids, edge_pose, plane_pose;
    std::vector<double> imu_c, vis_c, icp_c, lps_c, edge_c, plane_c;
    std::vector<char> pose_t(K, 0), sb_t(K, 0);
    bool ex_t = false, td_t = false;
    int n_lm_elim = 0;
    if (p->prior.n > 0) {
        bool has_drop = false;
        for (int b = 0; b < p->prior.nblk; ++b) {
            const int kind = p->prior.blk_kind[b], idx = p->prior.blk_index[b];
            if (kind == VIL_BLK_POSE) { pose_t[idx] = 1; if (idx == drop_pose) has_drop = true; }
            else if (kind == VIL_BLK_SPEEDBIAS) sb_t[idx] = 1;
            else if (kind == VIL_BLK_EX) ex_t = true; else td_t = true;
        }
        if (!old_ && !has_drop) { out->n = -1; return VIL_OK; }     // estimator.cpp:1620-1621: prior kept as is
    } else if (!old_) { out->n = -1; return VIL_OK; }
    if (old_) {
        for (int f = 0; f < p->n_imu; ++f) if (p->imu_i[f] == 0 && p->imu_j[f] == 1 && p->imu_const[(size_t)f * 287 + 16] < 10.0) {
            imu_i.push_back(0); imu_j.push_back(1); imu_c.insert(imu_c.end(), p->imu_const + (size_t)f * 287, p->imu_const + (size_t)(f + 1) * 287);
            pose_t[0] = pose_t[1] = 1; sb_t[0] = sb_t[1] = 1;
        }
        int last_l = -1;
        for (int f = 0; f < p->n_vis; ++f) if (p->vis_i[f] == 0) {
            vis_i.push_back(0); vis_j.push_back(p->vis_j[f]); vis_l.push_back(p->vis_l[f]);
            vis_c.insert(vis_c.end(), p->vis_const + (size_t)f * 14, p->vis_const + (size_t)(f + 1) * 14);
            pose_t[0] = 1; pose_t[p->vis_j[f]] = 1; ex_t = true; if (p->use_td) td_t = true;
            if (p->vis_l[f] != last_l) { ++n_lm_elim; last_l = p->vis_l[f]; }
        }
        if (spec->icp_marg >= 0 && spec->icp_marg < p->n_icp) {
            for (int b = 0; b < 4; ++b) { const int id = b == 0 ? 0 : p->icp_ids[4 * spec->icp_marg + b]; icp_ids.push_back(id); pose_t[id] = 1; }
            icp_c.insert(icp_c.end(), p->icp_const + (size_t)spec->icp_marg * 10, p->icp_const + (size_t)(spec->icp_marg + 1) * 10);
        }
        if (spec->lps_marg >= 0 && spec->lps_marg < p->n_lps) {
            for (int b = 0; b < 2; ++b) { const int id = b == 0 ? 0 : p->lps_ids[2 * spec->lps_marg + b]; lps_ids.push_back(id); pose_t[id] = 1; }
            lps_c.insert(lps_c.end(), p->lps_const + (size_t)spec->lps_marg * 7, p->lps_const + (size_t)(spec->lps_marg + 1) * 7);
        }
        // LiDAR point factors of the dropped pose (extended mode): MarginalizationInfo folds every factor that touches a
        // dropped block (marginalization_factor.cpp:176-316); these touch pose 0 only and reach the prior through A_mm / b_m
        for (int f = 0; f < p->n_edge; ++f) if (p->edge_pose[f] == 0) { edge_pose.push_back(0); edge_c.insert(edge_c.end(), p->edge_const + (size_t)f * 9, p->edge_const + (size_t)(f + 1) * 9); }
        for (int f = 0; f < p->n_plane; ++f) if (p->plane_pose[f] == 0) { plane_pose.push_back(0); plane_c.insert(plane_c.end(), p->plane_const + (size_t)f * 7, p->plane_const + (size_t)(f + 1) * 7); }
        if (!edge_pose.empty() || !plane_pose.empty()) pose_t[0] = 1;
    }
    q.n_imu = (int)imu_i.size(); q.imu_i = imu_i.data(); q.imu_j = imu_j.data(); q.imu_const = imu_c.data();
    q.n_vis = (int)vis_i.size(); q.vis_i = vis_i.data(); q.vis_j = vis_j.data(); q.vis_l = vis_l.data(); q.vis_const = vis_c.data();
    q.n_icp = (int)icp_ids.size() / 4; q.icp_ids = icp_ids.data(); q.icp_const = icp_c.data();
    q.n_lps = (int)lps_ids.size() / 2; q.lps_ids = lps_ids.data(); q.lps_const = lps_c.data();
    q.n_edge = (int)edge_pose.size(); q.edge_pose = edge_pose.data(); q.edge_const = edge_c.data();
    q.n_plane = (int)plane_pose.size(); q.plane_pose = plane_pose.data(); q.plane_const = plane_c.data();
    // under a communicator the collected factors are sharded like a solve's (visual by landmark owner, LiDAR points in slices, the rest on
    // rank 0), A and b are all-reduced ONCE and every rank finishes the small dense part redundantly -- the reference's own pattern
    // (marginalization_factor.cpp:235-264: factors dealt to four threads, private A / b, summed after the join)
    int st = (c->comm.sharded()) ? upload_sharded(c, &q, s) : upload_impl(c, &q, s, false);
    if (st != VIL_OK) return st;
    const SolveOpts so = to_dev_opts(o);
    st = init_ctl(c, o, 2);
    if (st != VIL_OK) return st;
    launch_sweep(c, so);
    st = launch_reduce_step(c, so, false);
    if (st != VIL_OK) return st;
    c->resident_kind = 2;
    return marg_finish(c, K, old_, drop_pose, pose_t, sb_t, ex_t, td_t, p->use_td != 0, n_lm_elim, s, out);
}

int vil_gauge_fix(const double* pose0_before, vil_state* s) {
    if (!pose0_before || !s) return VIL_ERR_INVALID_ARGUMENT;
    gauge_fix_core(pose0_before, s->K, s->pose, s->speedbias, s->ex_pose);
    return VIL_OK;
}

// visual factors by landmark owner (contiguous landmark ranges balanced by factor count),
// LiDAR points in contiguous equal chunks.  Pure host logic, no device needed.
int vil_shard_ranges(const vil_problem* p, int rank, int world, int32_t* lm_begin, int32_t* lm_end, int32_t* edge_begin, int32_t* edge_end, int32_t* plane_begin, int32_t* plane_end) {
    if (!p || world <= 0 || rank < 0 || rank >= world) return VIL_ERR_INVALID_ARGUMENT;
    std::vector<int> lms(p->L + 1, 0);
    for (int f = 0; f < p->n_vis; ++f) lms[p->vis_l[f] + 1]++;
    for (int l = 0; l < p->L; ++l) lms[l + 1] += lms[l];
    if (lm_begin) *lm_begin = shard_cut(lms, p->L, rank, world);
    if (lm_end) *lm_end = shard_cut(lms, p->L, rank + 1, world);
    if (edge_begin) *edge_begin = (int)((long long)p->n_edge * rank / world);
    if (edge_end) *edge_end = (int)((long long)p->n_edge * (rank + 1) / world);
    if (plane_begin) *plane_begin = (int)((long long)p->n_plane * rank / world);
    if (plane_end) *plane_end = (int)((long long)p->n_plane * (rank + 1) / world);
    return VIL_OK;
}

int vil_comm_message_bytes(vil_ctx* c, int64_t* bytes_per_peer, int64_t* bytes_full_set) {
    if (!c || !c->uploaded || !c->split) return VIL_ERR_INVALID_ARGUMENT;
    c->comm.message_bytes(c->D, c->span, bytes_per_peer, bytes_full_set);
    return VIL_OK;
}

// ---- window residency across frames (include/vilsolve.h) ------------------------------------------------------------------------
int vil_comm_info(vil_ctx* c, int32_t* rank, int32_t* world, int32_t* transport) {
    if (!c) return VIL_ERR_INVALID_ARGUMENT;
    if (rank) *rank = c->comm.rank;
    if (world) *world = c->comm.world;
    if (transport) *transport = c->comm.transport();
    return VIL_OK;
}
int vil_set_gauge_fix(vil_ctx* c, int32_t on) { if (!c) return VIL_ERR_INVALID_ARGUMENT; c->gauge_on = on != 0; return VIL_OK; }      // (takes effect in the next solve)

int vil_lidar_reset(vil_ctx* c) {
    if (!c) return VIL_ERR_INVALID_ARGUMENT;
    c->lidar.reset();
    if (c->lidar_resident) c->invalidate();      // the resident window's chunk list points into the old slab order
    return VIL_OK;
}
int vil_lidar_count(vil_ctx* c, int32_t* n_slabs, int32_t* n_plane, int32_t* n_edge) {
    if (!c) return VIL_ERR_INVALID_ARGUMENT;
    int np = 0, ne = 0;
    c->lidar.totals(&np, &ne);
    if (n_slabs) *n_slabs = c->lidar.count(); if (n_plane) *n_plane = np; if (n_edge) *n_edge = ne;
    return VIL_OK;
}
int vil_lidar_drop(vil_ctx* c, int32_t slab) {
    if (!c || slab < 0 || slab >= c->lidar.count()) return VIL_ERR_INVALID_ARGUMENT;
    c->lidar.drop(slab);
    if (c->lidar_resident) c->invalidate();      // slab <-> pose changed under the resident window's chunk list
    return VIL_OK;
}
int vil_lidar_push(vil_ctx* c, int32_t n_plane, const double* plane_const, int32_t n_edge, const double* edge_const) {
    if (!c || n_plane < 0 || n_edge < 0 || (n_plane > 0 && !plane_const) || (n_edge > 0 && !edge_const)) return VIL_ERR_INVALID_ARGUMENT;
    HIPCHK(hipSetDevice(c->device));
    const bool sh = c->comm.sharded();
    bool tables_moved = false;
    const int st = c->lidar.push(c->stream, sh ? c->comm.rank : 0, sh ? c->comm.world : 1, n_plane, plane_const, n_edge, edge_const, &tables_moved);
    if (tables_moved) c->uploaded = false;       // a resident problem holds pointers / strides of the old tables
    if (st != VIL_OK) return st;
    if (c->lidar_resident) c->invalidate();      // (a recycled slot would feed this frame's points to the old pose)
    return VIL_OK;
}

static int marginalize_resident_impl(vil_ctx* c, const vil_state* s, const vil_options* o, const vil_marg_spec* spec, vil_prior_out* out, const bool to_slot, vil_win_prior_info* winfo) {
    if (!c || !o || !spec || (!to_slot && (!s || !out)) || !c->uploaded || c->resident_kind != 1) return VIL_ERR_INVALID_ARGUMENT;
    const int K = c->K;
    if (K < 3 || (s && (s->K != K || s->L != c->L))) return VIL_ERR_INVALID_ARGUMENT;
    int none = 0; int& out_n = out ? out->n : none;
    HIPCHK(hipSetDevice(c->device));
    const vil_ctx::MargMeta& mm = c->mm;
    const bool old_ = spec->flag == VIL_MARGIN_OLD;
    const int drop_pose = old_ ? 0 : K - 2;
    std::vector<char> pose_t(K, 0), sb_t(K, 0);
    bool ex_t = false, td_t = false;
    int n_lm_elim = 0;
    if (mm.has_prior) {
        bool has_drop = false;
        for (size_t b = 0; b < mm.prior_kind.size(); ++b) {
            const int kind = mm.prior_kind[b], idx = mm.prior_index[b];
            if (kind == VIL_BLK_POSE) { pose_t[idx] = 1; if (idx == drop_pose) has_drop = true; }
            else if (kind == VIL_BLK_SPEEDBIAS) sb_t[idx] = 1;
            else if (kind == VIL_BLK_EX) ex_t = true; else td_t = true;
        }
        if (!old_ && !has_drop) { out_n = -1; if (winfo) winfo->n = -1; return VIL_OK; }     // estimator.cpp:1620-1621: prior kept as is
    } else if (!old_) { out_n = -1; if (winfo) winfo->n = -1; return VIL_OK; }
    int icp_m = -1, lps_m = -1;
    if (old_) {
        if (mm.imu01) { pose_t[0] = pose_t[1] = 1; sb_t[0] = sb_t[1] = 1; }
        if (mm.n_lm0 > 0) { pose_t[0] = 1; for (int k = 0; k < K; ++k) if (mm.obs0[k]) pose_t[k] = 1; ex_t = true; if (mm.use_td) td_t = true; n_lm_elim = mm.n_lm0; }
        if (spec->icp_marg >= 0 && 4 * (size_t)spec->icp_marg + 3 < mm.icp_ids.size()) {
            icp_m = spec->icp_marg;
            if (mm.icp_ids[4 * icp_m] != 0) return VIL_ERR_UNSUPPORTED;      // the remembered constraint starts in frame 0 (estimator.cpp:1381-1389)
            for (int b = 0; b < 4; ++b) pose_t[mm.icp_ids[4 * icp_m + b]] = 1;
        }
        if (spec->lps_marg >= 0 && 2 * (size_t)spec->lps_marg + 1 < mm.lps_ids.size()) {
            lps_m = spec->lps_marg;
            if (mm.lps_ids[2 * lps_m] != 0) return VIL_ERR_UNSUPPORTED;
            for (int b = 0; b < 2; ++b) pose_t[mm.lps_ids[2 * lps_m + b]] = 1;
        }
        if (mm.lidar0) pose_t[0] = 1;
    }
    const SolveOpts so = to_dev_opts(o);
    int st = init_ctl(c, o, 2);
    if (st != VIL_OK) return st;
    const DevP keep = c->P;
    c->P.marg = old_ ? 1 : 2; c->P.marg_icp = icp_m; c->P.marg_lps = lps_m;
    launch_sweep(c, so);                               // the resident tables at the resident (solved, gauge-fixed) state; masks select the factors
    st = launch_reduce_step(c, so, false);             // (sharded: A and b of this rank's factors, all-reduced once)
    c->P = keep;
    if (st != VIL_OK) return st;
    c->resident_kind = 2;                              // the work space now holds the marginalisation's linearisation
    return marg_finish(c, K, old_, drop_pose, pose_t, sb_t, ex_t, td_t, mm.use_td, n_lm_elim, s, out, to_slot, winfo);
}
int vil_marginalize_resident(vil_ctx* c, const vil_state* s, const vil_options* o, const vil_marg_spec* spec, vil_prior_out* out) {
    return marginalize_resident_impl(c, s, o, spec, out, false, nullptr);
}

// ---- the fully resident window (include/vilsolve.h: vil_win_*; device side: vil_window.hpp) ------------------------------------------
int vil_win_open(vil_ctx* c, const vil_win_cfg* cfg) {
    if (!c || !cfg || cfg->K < 3 || cfg->K > VIL_WIN_MAXK || cfg->max_tracks < 1 || cfg->max_samples < 1) return VIL_ERR_INVALID_ARGUMENT;
    if (c->comm.world > 1 && !c->comm.ready()) return VIL_ERR_COMM;
    HIPCHK(hipSetDevice(c->device));
    const int st = c->win.open(c->stream, cfg);
    if (st != VIL_OK) return st;
    c->invalidate();
    return vil_lidar_reset(c);
}

int vil_win_push_frame(vil_ctx* c, const vil_win_frame* f) {
    if (!c || !f || !c->win.is_open) return VIL_ERR_INVALID_ARGUMENT;
    Window& w = c->win;
    if (w.frames() >= w.K || f->n_samples < 0 || f->n_samples > w.S || f->n_obs < 0 || f->n_obs > w.T) return VIL_ERR_INVALID_ARGUMENT;
    if ((f->n_samples > 0 && (!f->dt || !f->acc || !f->gyr)) || (f->n_obs > 0 && (!f->obs_track || !f->obs))) return VIL_ERR_INVALID_ARGUMENT;
    for (int q = 0; q < f->n_obs; ++q) if (f->obs_track[q] < 0 || f->obs_track[q] >= w.T) return VIL_ERR_INVALID_ARGUMENT;
    // (the LiDAR arguments are checked BEFORE the frame / IMU slots are committed: a frame whose points fail must not leave fslot one entry ahead of
    //  the slabs -- "slab i <-> pose K - count + i" would then attach every later frame's points to the wrong pose)
    if (f->n_plane < 0 || f->n_edge < 0 || (f->n_plane > 0 && !f->plane_const) || (f->n_edge > 0 && !f->edge_const)) return VIL_ERR_INVALID_ARGUMENT;
    HIPCHK(hipSetDevice(c->device));
    const int st = w.push_frame(c->stream, f);
    if (st != VIL_OK) return st;
    c->invalidate();
    const int lst = vil_lidar_push(c, f->n_plane, f->plane_const, f->n_edge, f->edge_const);
    if (lst != VIL_OK) w.unpush_frame();                 // (an allocation failed): the frame is taken back -- slots returned, nothing refers to what its kernels wrote
    return lst;
}

int vil_win_drop_frame(vil_ctx* c, int32_t flag) {
    if (!c || !c->win.is_open) return VIL_ERR_INVALID_ARGUMENT;
    if (c->win.frames() < 2) return VIL_ERR_INVALID_ARGUMENT;
    HIPCHK(hipSetDevice(c->device));
    c->invalidate();
    int slab = 0;
    const int st = c->win.drop_frame(c->stream, flag, &slab);
    return st != VIL_OK ? st : vil_lidar_drop(c, slab);
}

int vil_win_solve(vil_ctx* c, const vil_win_problem* wp, vil_state* s, const vil_options* o, vil_summary* sum) {
    if (!c || !wp || !s || !o || !sum || !c->win.is_open) return VIL_ERR_INVALID_ARGUMENT;
    const Window& w = c->win;
    const int K = w.K, L = wp->L;
    if (w.frames() != K || L < 0 || s->K != K || s->L != L) return VIL_ERR_INVALID_ARGUMENT;
    if (L > 0 && (!wp->lm_track || !wp->lm_start || !wp->lm_nobs)) return VIL_ERR_INVALID_ARGUMENT;
    int n_vis = 0;
    for (int l = 0; l < L; ++l) {
        if (wp->lm_track[l] < 0 || wp->lm_track[l] >= w.T || wp->lm_start[l] < 0 || wp->lm_nobs[l] < 2 || wp->lm_start[l] + wp->lm_nobs[l] > K) return VIL_ERR_INVALID_ARGUMENT;
        n_vis += wp->lm_nobs[l] - 1;
    }
    const auto t0 = std::chrono::steady_clock::now();
    vil_problem q; memset(&q, 0, sizeof q);
    q.K = K; q.L = L; q.pose_const = wp->pose_const; q.sb_const = wp->sb_const; q.lm_const = wp->lm_const;
    q.ex_const = wp->ex_const; q.td_const = wp->td_const; q.use_td = w.cfg.use_td;
    int imu_i[VIL_WIN_MAXK], imu_j[VIL_WIN_MAXK];
    for (int k = 0; k + 1 < K; ++k) { imu_i[k] = k; imu_j[k] = k + 1; }
    q.n_imu = K - 1; q.imu_i = imu_i; q.imu_j = imu_j; q.imu_const = nullptr;
    w.prior_blocks(q.prior);
    q.n_icp = wp->n_icp; q.icp_ids = wp->icp_ids; q.icp_const = wp->icp_const; q.n_lps = wp->n_lps; q.lps_ids = wp->lps_ids; q.lps_const = wp->lps_const;
    q.n_plane = q.n_edge = VIL_LIDAR_RESIDENT;
    memcpy(q.q_lb, w.cfg.q_lb, sizeof q.q_lb); memcpy(q.t_lb, w.cfg.t_lb, sizeof q.t_lb); memcpy(q.G, w.cfg.G, sizeof q.G);
    q.sqrt_info_px = w.cfg.sqrt_info_px; q.tr_over_row = w.cfg.tr_over_row;
    WinSrc ws; memset(&ws, 0, sizeof ws);
    ws.lm_track = wp->lm_track; ws.lm_startf = wp->lm_start; ws.lm_nobs = wp->lm_nobs; ws.n_vis = n_vis;
    w.fill(ws);
    ws.lb = 0; ws.le = L; ws.f0 = 0; ws.n_vis_all = n_vis;
    // vil_win_solve returns the gauge-fixed state and vil_win_marginalize linearises at it (double2vector() precedes the marginalisation,
    // estimator.cpp:1419 / :1487): the device gauge fix is part of the resident window whatever vil_set_gauge_fix was left at
    const bool gauge_was = c->gauge_on; c->gauge_on = true;
    int st;
    if (c->comm.sharded()) {
        // SURVEY 8e on the resident window: every rank was handed every frame (vil_win_push_frame: the observation store and the IMU slots are whole on
        // every rank, the LiDAR slabs hold the rank's slice) and is handed the same small tables here; it keeps the visual factors of ITS landmark range
        // -- the rule of vil_shard_ranges on the landmark list -- and rank 0 alone the IMU / prior / ICP / LPS factors.  The prior slot is written by
        // every rank from the all-reduced marginalisation system (identical bits), read by rank 0.
        std::vector<int> lms(L + 1, 0);
        for (int l = 0; l < L; ++l) lms[l + 1] = lms[l] + wp->lm_nobs[l] - 1;
        Comm& cm = c->comm;
        cm.set_owners(lms, L, K);
        ws.lb = shard_cut(lms, L, cm.rank, cm.world); ws.le = shard_cut(lms, L, cm.rank + 1, cm.world); ws.f0 = lms[ws.lb]; ws.n_vis = lms[ws.le] - lms[ws.lb];
        vil_problem ql = q;
        if (cm.rank != 0) { ql.n_imu = 0; ql.n_icp = 0; ql.n_lps = 0; ql.prior.n = 0; ql.prior.nblk = 0; }
        st = cm.agree(c->stream, upload_impl(c, &ql, s, true, nullptr, &q, ws.f0, false, &ws));
        if (st != VIL_OK) c->uploaded = false;
    } else st = upload_impl(c, &q, s, false, nullptr, nullptr, 0, false, &ws);
    if (st != VIL_OK) { c->gauge_on = gauge_was; return st; }
    c->resident_kind = 1;
    c->P.setup_stat = w.status_word();                      // the window's sticky status word: a failed pre-integration / prior ends the solve with it
    const auto t1 = std::chrono::steady_clock::now();
    st = vil_solve_resident(c, o, sum);
    c->gauge_on = gauge_was;                           // (the caller's setting governs vil_solve / vil_solve_resident of other uploads again)
    sum->t_prepare_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
    if (st != VIL_OK) return st;                       // state left unchanged on any error
    const auto t2 = std::chrono::steady_clock::now();
    st = vil_download_state(c, s);
    sum->t_readback_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t2).count();
    return st;
}

int vil_win_marginalize(vil_ctx* c, const vil_options* o, const vil_marg_spec* spec, vil_win_prior_info* info) {
    if (!c || !c->win.is_open) return VIL_ERR_INVALID_ARGUMENT;
    return marginalize_resident_impl(c, nullptr, o, spec, nullptr, true, info);
}

int vil_win_prior_download(vil_ctx* c, vil_prior_out* out) {
    if (!c || !out || !c->win.is_open) return VIL_ERR_INVALID_ARGUMENT;
    HIPCHK(hipSetDevice(c->device));
    return c->win.prior_download(c->stream, out, &c->h_word.p[8]);
}

int vil_win_prior_set(vil_ctx* c, const vil_prior* pr) {
    if (!c || !c->win.is_open) return VIL_ERR_INVALID_ARGUMENT;
    HIPCHK(hipSetDevice(c->device));
    if (pr && pr->n > 0 && (pr->n > c->win.nmax || pr->nblk <= 0 || pr->nblk > VIL_WIN_MAXBLK || !pr->blk_kind || !pr->blk_index || !pr->blk_col || !pr->x0 || !pr->J0 || !pr->r0)) return VIL_ERR_INVALID_ARGUMENT;
    return c->win.prior_set(c->stream, pr);      // (a prior whose x0 exceeds the slot's capacity is an invalid argument as well)
}

// ---- multi-GPU set-up (vil_comm.hpp): installing a transport releases whatever the context had, and invalidates the resident problem
int vil_comm_unique_id(void* id128) { return id128 ? Comm::unique_id(id128) : VIL_ERR_INVALID_ARGUMENT; }
int vil_comm_init(vil_ctx* c, const void* id128, int rank, int world) {
    if (!c || !id128 || world < 1 || rank < 0 || rank >= world) return VIL_ERR_INVALID_ARGUMENT;
    HIPCHK(hipSetDevice(c->device));
    c->uploaded = false;
    return c->comm.use_rccl(c->device, id128, rank, world);
}
int vil_comm_ipc_export(vil_ctx* c, int rank, int world, size_t max_doubles, void* handle64) {
    if (!c || !handle64 || world < 1 || world > 8 || rank < 0 || rank >= world || max_doubles < 64) return VIL_ERR_INVALID_ARGUMENT;
    HIPCHK(hipSetDevice(c->device)); HIPCHK(hipStreamSynchronize(c->stream));
    c->uploaded = false;
    return c->comm.export_ipc(c->device, rank, world, max_doubles, handle64);
}
int vil_comm_ipc_init(vil_ctx* c, const void* handles) {
    if (!c || !handles) return VIL_ERR_INVALID_ARGUMENT;
    HIPCHK(hipSetDevice(c->device));
    return c->comm.open_ipc(handles);
}
int vil_comm_init_local(vil_ctx** ctxs, int n) {
    if (!ctxs || n < 1 || n > 8) return VIL_ERR_INVALID_ARGUMENT;
    Comm* ranks[8]; int devices[8];
    for (int r = 0; r < n; ++r) { if (!ctxs[r]) return VIL_ERR_INVALID_ARGUMENT; ranks[r] = &ctxs[r]->comm; devices[r] = ctxs[r]->device; }
    const int st = Comm::join_local(ranks, devices, n);
    if (st == VIL_OK) for (int r = 0; r < n; ++r) ctxs[r]->uploaded = false;
    return st;
}

// ---- the lab bench (include/vilsolve_debug.h): test hooks and the profilers of the kernels' role layout ------------------------------------------
int vil_debug_set_launch_mode(vil_ctx* c, int32_t mode) { if (!c || mode < 0 || mode > 4) return VIL_ERR_INVALID_ARGUMENT; c->launch_mode = mode; c->invalidate(); return VIL_OK; }
int vil_debug_get_launch_structure(vil_ctx* c, int32_t* launches_per_iteration, int32_t* one_launch) {
    if (!c || !c->uploaded) return VIL_ERR_INVALID_ARGUMENT;
    const int rung = top_rung(c);
    if (launches_per_iteration) *launches_per_iteration = rung < 2 ? rung : (c->ls.rs_merged != 0 && !c->split ? 2 : 3);      // 0: the whole solve is one resident launch (k_solve)
    if (one_launch) *one_launch = rung < 2 ? 1 : 0;
    return VIL_OK;
}
int vil_debug_fail_graph_capture(vil_ctx* c, int32_t n) { if (!c || n < 0) return VIL_ERR_INVALID_ARGUMENT; c->fail_capture = n; c->graph_failed = false; return VIL_OK; }
int vil_debug_drop_flag(vil_ctx* c, int32_t role, int32_t launch) {
    if (!c || launch < 0) return VIL_ERR_INVALID_ARGUMENT;
    c->drop_role = role; c->drop_launch = launch;
    return VIL_OK;
}
int vil_debug_set_split(vil_ctx* c, int32_t on) { if (!c) return VIL_ERR_INVALID_ARGUMENT; c->force_split = on != 0; c->invalidate(); return VIL_OK; }
int vil_debug_set_slim_emul(vil_ctx* c, int32_t on) { if (!c) return VIL_ERR_INVALID_ARGUMENT; c->comm.slim_emul = on != 0; return VIL_OK; }
// WW != null: the matrix is A - S WW S, subtracted on the factorisation's register tiles out of the lane-major tile layout (vil_debug_dense_solve_ww)
static int debug_dense_run(vil_ctx* c, int32_t D, const double* A, const double* WW, const double* sc, double pad, double* L, double* x, int32_t* ok, int32_t variant) {
    if (!c || !A || !L || !x || !ok || D < 1 || D > 159 || variant < 0 || variant > 1) return VIL_ERR_INVALID_ARGUMENT;
    HIPCHK(hipSetDevice(c->device));
    const int R = D + 1, T = (R + 15) / 16, nt = T * (T + 1) / 2;
    const size_t lds = 8 * (size_t)TILE_SZ * nt, nb = 8 * (size_t)R * R;
    const size_t nRR = (size_t)R * R;
    vilhost::Grown<double> tA, tL, tx, tW, tWW, tsc; vilhost::Grown<int> tok;      // (freed on every return)
    HIPCHK(tA.reserve(nRR, nRR)); HIPCHK(tL.reserve(nRR, nRR)); HIPCHK(tx.reserve(R, R)); HIPCHK(tok.reserve(16, 16));
    double *dA = tA.p, *dL = tL.p, *dx = tx.p, *dW = nullptr, *dWW = nullptr, *dsc = nullptr; int* dok = tok.p;
    HIPCHK(hipMemcpy(dA, A, nb, hipMemcpyHostToDevice));
    const void* fn;
    if (WW) {
        HIPCHK(tW.reserve(nRR, nRR)); HIPCHK(tWW.reserve((size_t)256 * nt, (size_t)256 * nt)); HIPCHK(tsc.reserve(D, D));
        dW = tW.p; dWW = tWW.p; dsc = tsc.p;
        HIPCHK(hipMemcpy(dW, WW, nb, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(dsc, sc, 8 * (size_t)D, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_debug_ww_fill, dim3(nt), dim3(256), 0, c->stream, dW, dWW, D, pad);
        const bool small = nt <= 24;                     // (the step's own choice: solve_prechain)
        fn = variant ? (small ? (const void*)k_debug_dense<3, true, true> : (const void*)k_debug_dense<CH_SLOTS, true, true>) : (small ? (const void*)k_debug_dense<3, false, true> : (const void*)k_debug_dense<CH_SLOTS, false, true>);
    } else {
        const bool small = nt <= 18;                     // (three register tiles per tile wave are enough -- what the step takes at K <= 10)
        fn = variant ? (small ? (const void*)k_debug_dense<3, true> : (const void*)k_debug_dense<CH_SLOTS, true>) : (small ? (const void*)k_debug_dense<3, false> : (const void*)k_debug_dense<CH_SLOTS, false>);
    }
    HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    void* args[] = {(void*)&dA, (void*)&dL, (void*)&dx, (void*)&dok, (void*)&D, (void*)&dWW, (void*)&dsc};
    HIPCHK(hipLaunchKernel(fn, dim3(1), dim3(VIL_STEP_THREADS), args, lds, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    int hok = 0;
    HIPCHK(hipMemcpy(L, dL, nb, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(x, dx, 8 * (size_t)D, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(&hok, dok, 4, hipMemcpyDeviceToHost));
    *ok = hok;
    return VIL_OK;
}
int vil_debug_dense_solve(vil_ctx* c, int32_t D, const double* A, double* L, double* x, int32_t* ok, int32_t variant) { return debug_dense_run(c, D, A, nullptr, nullptr, 0.0, L, x, ok, variant); }
int vil_debug_dense_solve_ww(vil_ctx* c, int32_t D, const double* A, const double* WW, const double* sc, double pad, double* L, double* x, int32_t* ok, int32_t variant) {
    if (!WW || !sc) return VIL_ERR_INVALID_ARGUMENT;
    return debug_dense_run(c, D, A, WW, sc, pad, L, x, ok, variant);
}
int vil_debug_read(vil_ctx* c, long long* out64) {
    if (!c || !c->uploaded) return VIL_ERR_INVALID_ARGUMENT;
    HIPCHK(hipMemcpy(out64, c->P.dbg, 8 * 64, hipMemcpyDeviceToHost));
    return VIL_OK;
}
/* average position (us after the launch's first workgroup started) of the phase stamps of the one-launch iterations timed since the last reset:
 * [0] 0, [1] last visual / LiDAR / ICP-LPS role done, [2] last IMU role done, [3] chain: records seen, [4] chain: W^T complete, [5] last gather workgroup done,
 * [6] last gather workgroup saw the visual flags, [7] master started, [8] master saw the gather's flags, [9] master saw the W W^T tiles,
 * [10] dense factorisation done, [11] x_p published, [12] master done, [13] last tile workgroup done, [14] chain: its part of S' gathered, [15] prior role done,
 * [16 .. 20] IMU role of factor 0: entered, inputs staged, raw blocks done, whitened, record stores issued; [21 .. 23] master: chain back-substituted (solve done),
 * step vectors + helpers' sums in, candidate formed */
int vil_profile_phases(vil_ctx* c, double* avg_us, int64_t* launches, int reset) {
    if (!c || !avg_us) return VIL_ERR_INVALID_ARGUMENT;
    for (int k = 0; k < VIL_PROF_SLOTS; ++k) avg_us[k] = c->phase_n ? c->phase_us[k] / (double)c->phase_n : 0.0;
    avg_us[0] = c->period_n ? c->phase_us[0] / (double)c->period_n : 0.0;      // [0]: average iteration period inside a persistent solve (0: launches)
    if (launches) *launches = c->phase_n;
    if (reset) { for (double& v : c->phase_us) v = 0.0; c->phase_n = 0; c->period_n = 0; }
    return VIL_OK;
}
int vil_profile_workgroups(vil_ctx* c, int32_t launch, uint64_t* times, int32_t max_workgroups) {
    if (!c) return VIL_ERR_INVALID_ARGUMENT;
    if (!times) {                                         // arm: the solves from now on record launch `launch` (< 0: none)
        c->wg_launch = launch;
        if (c->d_prof.p) { HIPCHK(hipStreamSynchronize(c->stream)); HIPCHK(hipMemset((char*)c->d_prof.p + 8 * 64 * VIL_PROF_SLOTS, 0, 8 * 2 * VIL_PROF_WGS)); }
        return VIL_OK;
    }
    if (!c->d_prof.p || max_workgroups < 0) return VIL_ERR_INVALID_ARGUMENT;
    HIPCHK(hipStreamSynchronize(c->stream));
    const int n = std::min<int>(max_workgroups, VIL_PROF_WGS);
    HIPCHK(hipMemcpy(times, (char*)c->d_prof.p + 8 * 64 * VIL_PROF_SLOTS, 8 * 2 * (size_t)n, hipMemcpyDeviceToHost));
    return VIL_OK;
}
int vil_debug_read_stamps(vil_ctx* c, uint64_t* out, int32_t max_launches) {
    if (!c || !out || max_launches < 0) return VIL_ERR_INVALID_ARGUMENT;
    const size_t n = std::min((size_t)max_launches * VIL_PROF_SLOTS, c->last_stamps.size());
    for (size_t i = 0; i < n; ++i) out[i] = c->last_stamps[i];
    return (int)(n / VIL_PROF_SLOTS);
}
int vil_debug_marg_stamps(vil_ctx* c, uint64_t* out16) {
    if (!c || !out16 || !c->d_marg_ts) return VIL_ERR_INVALID_ARGUMENT;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(out16, c->d_marg_ts, 8 * 16, hipMemcpyDeviceToHost));
    return VIL_OK;
}

}  // extern "C"
