/*
 * vilsolve_debug_ww.h -- one more test hook of libvilsolve.so's lab bench (vilsolve_debug.h), declared on its own: the step's dense solve
 * together with the subtraction of the chain's W W^T on the factorisation's register tiles.  tests/test_gpu_wwsub.py calls it.
 */
#ifndef VILSOLVE_DEBUG_WW_H
#define VILSOLVE_DEBUG_WW_H

#include "vilsolve_debug.h"

#ifdef __cplusplus
extern "C" {
#endif

/* test hook: the solve of vil_debug_dense_solve on A - S WW S, with the subtraction done the way the step takes the chain's W W^T off the pose system: WW ((D + 1) x (D + 1) row
 * major, EVERY entry is copied; tile elements past row / column D get `pad`) is written in the lane-major tile layout of the tile workgroups (vil_prechain.hpp,
 * ww_idx) and subtracted on the factorisation's register tiles before its first barrier -- rows i < D scaled by sc[i] sc[j], the right-hand-side row D by sc[j]
 * alone; entries above the diagonal, the entry (D, D) and the padding must not reach the result.  sc: D scales.  Everything else as vil_debug_dense_solve. */
int vil_debug_dense_solve_ww(vil_ctx* ctx, int32_t D, const double* A, const double* WW, const double* sc, double pad, double* L, double* x, int32_t* ok, int32_t variant);

#ifdef __cplusplus
}
#endif

#endif
