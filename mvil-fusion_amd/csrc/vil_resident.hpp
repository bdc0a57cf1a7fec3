// vil_resident.hpp -- what libvilsolve.so keeps on the device BETWEEN two images, behind two types (vilwindow.hip); internal, like vil_comm.hpp.
//   LidarSlabs   the LiDAR points of the window frames (vil_lidar_*): slab i <-> pose K - count + i, sliding the window is an index remap
//   Window       the fully resident window (vil_win_*; layout: vil_window.hpp): observation store, IMU slots, two prior slots
// Neither knows the solver's context: the entry points of vilsolve.hip validate, call a method with their stream, and invalidate the resident problem.
#pragma once
#include <hip/hip_runtime.h>
#include <vector>
#include "vil_host.hpp"
#include "vil_internal.h"
#include "vil_dev.hpp"

// a kept block of a prior: its doubles in x0 (pose / extrinsic 7, speed-bias 9, td 1), its tangent columns, and the address shift of
// slideWindow as an index remap (estimator.cpp:1599-1611, 1654-1677)
static inline int blk_doubles(int kind) { return (kind == VIL_BLK_POSE || kind == VIL_BLK_EX) ? 7 : (kind == VIL_BLK_SPEEDBIAS ? 9 : 1); }
static inline int blk_cols(int kind) { const int gs = blk_doubles(kind); return gs == 7 ? 6 : gs; }
static inline int blk_shift(int kind, int idx, bool old_, int K) { return (kind == VIL_BLK_POSE || kind == VIL_BLK_SPEEDBIAS) ? (old_ ? idx - 1 : (idx == K - 1 ? K - 2 : idx)) : idx; }

// what a solve reads of the window (Window::fill): the store, the slots of the window frames, the current prior slot
struct WinSlots {
    int T;
    const double* store; const int* fslot; const int* islot;            // slots of the window frames (host, K each)
    const double* d_rec; const double* d_U; const double* sum_dt;       // IMU slots (device) and the intervals' durations (host, per physical slot)
    const double* pJ0; const double* pr0; const double* px0; double* pH; double* pg0; double* pc0;     // device prior slot (prior.n > 0)
};

// One pushed frame travels as ONE DMA out of a pinned block into its device twin (both grow-only): fill h after begin(), then send()
struct __attribute__((visibility("hidden"))) FrameStage {
    vilhost::Grown<char, true> h; vilhost::Grown<char> d;
    int begin(hipStream_t stream, size_t bytes, size_t grow_to);      // the previous frame's DMA has left the pinned block; room for `bytes` (a new pair of grow_to bytes otherwise)
    int send(hipStream_t stream, size_t bytes);
private:
    vilhost::Fence sent;
};

struct __attribute__((visibility("hidden"))) LidarSlabs {
    int count() const { return (int)slabs.size(); }
    void totals(int* n_plane, int* n_edge) const;                       // points held (this rank's slices)
    bool frame0_has_points(int K) const;                                // by the UNSLICED counts: the same answer on every rank
    void chunks(bool plane, int K, std::vector<int>& out) const;        // appends (start, count <= VIL_THREADS, pose) per chunk, pose-ordered
    void tables(DevP& P) const;                                         // pl_c / pl_stride / ed_c / ed_stride
    void reset();
    void drop(int i);                                                   // the later frames move down: an index remap, the points stay where they are
    // the newest frame's points (point-major rows); of a sharded window (world > 1) this rank keeps its contiguous slice.  tables_moved: capacity grew,
    // the live slabs were copied into new tables -- a resident problem holds pointers / strides of the old ones
    int push(hipStream_t stream, int rank, int world, int n_plane, const double* plane, int n_edge, const double* edge, bool* tables_moved);
private:
    struct Slab { int np, ne, slot; int np_all, ne_all; };      // np_all / ne_all: the frame's points BEFORE a communicator's slicing (the same on every rank)
    std::vector<Slab> slabs;       // window order
    std::vector<int> free_slots;
    int cap_p = 0, cap_e = 0, nslot = 0;      // points per slab (capacity), physical slabs
    vilhost::Grown<double> d_pl, d_ed;                    // component-major: row q of the plane table at d_pl.p + q * nslot * cap_p
    FrameStage stage;              // AoS rows of one pushed frame
};

struct __attribute__((visibility("hidden"))) Window {
    bool is_open = false; vil_win_cfg cfg;
    int K = 0, T = 0, S = 0, nmax = 0, x0max = 0;      // frames, track slots, samples per interval; capacity of a prior slot (vil_prior_capacity)
    int frames() const { return (int)fslot.size(); }
    int open(hipStream_t stream, const vil_win_cfg* cfg);               // (re-)allocates when the dimensions change; an empty window without a prior
    int push_frame(hipStream_t stream, const vil_win_frame* f);         // observations into the store, samples into an IMU slot, its record and sqrt-information
    void unpush_frame();                                                // takes the newest frame's slots back (nothing refers to what its kernels wrote)
    int drop_frame(hipStream_t stream, int flag, int* lidar_slab);      // slideWindow; lidar_slab: the LiDAR slab that leaves with the frame
    void fill(WinSlots& ws) const;
    void prior_blocks(vil_prior& p) const;                              // n and the block tables of the current prior (host)
    // THE commit of a prior into the other slot, which then is the current one: J0 (n x n, column-major) | r0 from device memory, the contractions.
    // col == nullptr (marginalisation): index = the kept blocks' CURRENT frames -- x0 is gathered from the device state x, the tables get the slide's remap;
    // col != nullptr (vil_win_prior_set): x0 is in the slot already, the tables are taken as they are
    int commit_prior(hipStream_t stream, int K, bool old_, int n, int m, int nblk, const int* kind, const int* index, const int* col, const double* J0, const double* r0, const double* x);
    int prior_download(hipStream_t stream, vil_prior_out* out, int* h_word);      // returns the sticky status word
    int prior_set(hipStream_t stream, const vil_prior* pr);             // nullptr / n <= 0: no prior
    int* status_word() const { return d_wstat.p; }                        // sticky status of the asynchronous work (a covariance that is not positive definite, a prior that is not finite)
private:
    void release_tables();                                              // (open() with other dimensions)
    int NF = 0;
    std::vector<int> fslot, islot, free_f, free_i;           // window frame -> observation slot / IMU slot; free lists
    std::vector<int> ns; std::vector<double> sum_dt;          // per IMU slot: samples held, duration of the interval
    vilhost::Grown<double> d_store, d_samp, d_hdr, d_rec, d_U;
    vilhost::Grown<double> d_prior[2]; int cur = 0;               // prior slots: [J0 nmax^2 | r0 nmax | x0 x0max | pH nmax^2 | pg0 nmax | pc0 8]
    int pn = 0, pm = 0; std::vector<int> pkind, pindex, pcol;  // the current prior's block structure (host)
    vilhost::Grown<int> d_wstat;
    int lds_commit = 0;            // dynamic LDS k_prior_commit was granted
    FrameStage stage;              // [hdr 12 | dt | acc | gyr | observations | track slots] of one pushed frame
    double* dt(int q) const { return d_samp.p + (size_t)q * 7 * S; }
    double* acc(int q) const { return dt(q) + S; }
    double* gyr(int q) const { return dt(q) + 4 * (size_t)S; }
    double* pJ0(int w) const { return d_prior[w].p; }
    double* pr0(int w) const { return pJ0(w) + (size_t)nmax * nmax; }
    double* px0(int w) const { return pr0(w) + nmax; }
    double* pH(int w) const { return px0(w) + x0max; }
    double* pg0(int w) const { return pH(w) + (size_t)nmax * nmax; }
    double* pc0(int w) const { return pg0(w) + nmax; }
    size_t prior_doubles() const { return 2 * (size_t)nmax * nmax + 2 * (size_t)nmax + x0max + 8; }
};
