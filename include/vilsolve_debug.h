/*
 * vilsolve_debug.h -- the lab bench of libvilsolve.so: test hooks (vil_debug_*) and the profilers whose slot tables are the kernels'
 * internal role layout (vil_profile_phases, vil_profile_workgroups).  Tests, tools/ and bench.py call them; an integration of the
 * boundary (vilsolve.h) needs none of them.  Same library, same calling conventions and status codes.
 */
#ifndef VILSOLVE_DEBUG_H
#define VILSOLVE_DEBUG_H

#include "vilsolve.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- launch structure ------------------------------------------------------------------------- */
/* test hook: which launch structure a single-GPU solve takes.  0 (default): the library's choice -- the whole iteration (sweep, gather, chain elimination, step)
 * in ONE launch whenever the device holds its waiting workgroups and the roles share one dynamic-LDS size (every BASELINE size on an MI355X), else the next one
 * down this list; 3: sweep launch + gather / step launch (round 4's structure); 1: the fallback for devices / windows where it does not: separate gather launch, the speed-bias chain
 * eliminated by a workgroup of the SWEEP launch; 2: no chain workgroup at all (the step kernel eliminates the chain itself, the round-2 structure).
 * 4: one launch per ITERATION (k_iter) also where the whole solve could run as one resident launch (k_solve: the default for windows whose every role fits the
 * device at once -- configs[1]; same bits as mode 4).
 * Same results to rounding in every mode.  Invalidates the resident window. */
int vil_debug_set_launch_mode(vil_ctx* ctx, int32_t mode);
/* what the uploaded window's solves launch per trust-region iteration: 0 (nothing: the whole solve is ONE resident launch, k_solve -- windows whose roles all fit the
 * device at once; *one_launch = 1 as well), 1 (the one-launch iteration), 2 (sweep + gather / step) or 3 (sweep, gather, step) */
int vil_debug_get_launch_structure(vil_ctx* ctx, int32_t* launches_per_iteration, int32_t* one_launch);
/* test hook: the next n hipGraph captures of this context's solves are treated as failed (as a driver that cannot capture or instantiate the chunk would make them).
 * A failed capture is not an error: nothing has run yet, the solve at hand and every later solve of the context launch directly.  n = 0 re-arms graph replay. */
int vil_debug_fail_graph_capture(vil_ctx* ctx, int32_t n);
/* test hook for the recovery of a one-launch solve (vilsolve.h, vil_recovery_counts): in launch `launch` (0-based) of the NEXT solve, sweep role `role` (workgroup
 * index in the sweep's order [imu | prior | rel | visual | plane | edge]; -2 - g: gather workgroup g) does not post its completion flag -- what a workgroup that
 * never became resident looks like to the ones waiting for it.
 * launch | 0x10000: a gather workgroup's flag is lost in the retry as well (a solve that fails on both structures). */
int vil_debug_drop_flag(vil_ctx* ctx, int32_t role, int32_t launch);

/* ---- multi-GPU plumbing on one device ------------------------------------------------------------ */
/* test hook: run the multi-GPU plumbing (partial system in set 0, the collective sums it into set 1, step kernel on set 1) on a
 * single rank, with or without a 1-rank communicator.  Invalidates the resident window. */
int vil_debug_set_split(vil_ctx* ctx, int32_t on);
/* test hook: the pack / unpack kernels of the RCCL path (vilsolve.h, vil_comm_init) over the in-process communicator (two small kernels stand in for the RCCL
 * calls), so that they run on 2 / 3 / 8 ranks of one device. */
int vil_debug_set_slim_emul(vil_ctx* ctx, int32_t on);

/* ---- single pieces of a solve ------------------------------------------------------------------- */
/* test hook: the step's dense solve on a matrix of the caller's -- A is (D + 1) x (D + 1) row major, its lower triangle the SPD matrix, its last row the right-hand
 * side (D <= 159).  L receives the Cholesky factor (lower, row major, last row = L^-1 rhs), x the solution, *ok 0 when a pivot was not positive.  variant 1: what the
 * one-launch iteration runs (16-wide panels factored a matrix row per lane, back substitution a column per lane: vil_step.hpp chol_rowwave / back_subst_cols);
 * variant 0: the look-ahead factorisation (4-wide panels) and the back substitution through inverted diagonal tiles that the other launch structures run. */
int vil_debug_dense_solve(vil_ctx* ctx, int32_t D, const double* A, double* L, double* x, int32_t* ok, int32_t variant);
/* (the same solve with the chain's W W^T subtraction in front of it: vilsolve_debug_ww.h) */
/* the 64 words of the kernels' debug block (DevP::dbg: the clock stamps of the -DVIL_STAMPS build, tools/probe_step.py) of the uploaded window */
int vil_debug_read(vil_ctx* ctx, long long* out64);

/* ---- profilers of the kernels' role layout (vil_profile_enable, vilsolve.h) ---------------------------- */
/* One-launch iterations stamp their phases with the device's 100 MHz wall clock while profiling is on.  vil_profile_phases returns the average position in
 * microseconds of 16 phase stamps after the launch's first workgroup started (24 slots; csrc/vilsolve.hip lists them) and the number of launches averaged. */
int vil_profile_phases(vil_ctx* ctx, double* avg_us32, int64_t* launches, int reset);
/* profiling (with vil_profile_enable(ctx, 1), one-launch iterations): times == NULL arms it -- from now on every workgroup of launch `launch` (0-based) of a solve
 * leaves its entry and exit time (100 MHz device clock) --; with times != NULL the pairs {entry, exit} of the first max_workgroups (<= 4096) workgroups of the last
 * recorded launch are copied out, in block-index order = the launch's grid order [imu | prior | rel][chain][visual | plane | edge][master | helpers | tiles][gather]
 * (zeros: a workgroup that did not run).  tools/probe_workgroups.py prints them by role. */
int vil_profile_workgroups(vil_ctx* ctx, int32_t launch, uint64_t* times, int32_t max_workgroups);
/* the raw stamps (100 MHz device clock; 32 per launch / iteration, slot 0 stored inverted; 0: not stamped) of the last profiled solve: returns the launches copied */
int vil_debug_read_stamps(vil_ctx* ctx, uint64_t* out, int32_t max_launches);
/* the 16 wall-clock stamps (100 MHz) the kernels of the context's LAST marginalisation left: k_marg [0] entered, [1] dropped block gathered, [2] its Cholesky inverse
 * done, [3] kept x dropped blocks staged, [4] T = A_kd A_dd^-1, [5] A = A_kk - T A_dk and b, [6] symmetrised copies out; k_marg_fast [7] entered, [8] tiles loaded,
 * [9] n x n factorisation done, [10] J0 / r0 out; k_marg (pivoted square root, only when the un-pivoted one was refused) [11] entered, [12] done */
int vil_debug_marg_stamps(vil_ctx* ctx, uint64_t* out16);

#ifdef __cplusplus
}
#endif
#endif /* VILSOLVE_DEBUG_H */
