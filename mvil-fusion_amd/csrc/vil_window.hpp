// Device side of the fully resident window (include/vilsolve.h: vil_win_*).  What slideWindow() (estimator.cpp:1689-1814)
// leaves unchanged between two images stays in HBM, addressed by SLOTS that the host hands out and recycles -- sliding the window is
// an index remap on the host, nothing moves on the device:
//   observation store   obs[(frame slot * T + track slot) * 8 + c], c: x y z vx vy cur_td row -   (FeaturePerFrame, feature_manager.h:18-44)
//   IMU slots           raw samples (dt | acc | gyr), the interval's first measurement and bias linearisation point, its 287-double
//                       pre-integration record (k_preint writes it here) and the factored sqrt-information U (225)
//   LiDAR frame slabs   (vil_resident.hpp: LidarSlabs)
//   prior slots (2)     J0 | r0 | x0 | J0^T J0 | J0^T r0 | r0^T r0: written by the marginalisation kernels, read by the next solve
// Per image the host sends ONE packet with the new frame (samples, observations, LiDAR points) and one with the small index tables of
// the window; k_win_pack expands the landmark table into the factor tables the sweep reads.  The store itself -- slots, staging, the kernels that
// write it -- is the Window of vil_resident.hpp / vilwindow.hip; here is what the solver's upload launches.
#pragma once
#include "vil_dev.hpp"

#define VIL_WIN_OBS 8
#define VIL_WIN_MAXK 20

struct WinPack {
    // visual: landmark l = track slot lm_track[l], anchored in window frame lm_startf[l], factors lm_start[l] .. lm_start[l+1] (one per later observation)
    int L, F, stride, T;
    const int* lm_start; const int* lm_track; const int* lm_startf; const double* store;
    int fslot[VIL_WIN_MAXK];
    double* vis_c; int* vis_i; int* vis_j; int* vis_l; int* fcol; const int* vfinv;
    // IMU factor f = (f, f + 1): record and U of the IMU slot of frame f + 1
    int n_imu; const double* rec; const double* U; int islot[VIL_WIN_MAXK]; double* imu_c; double* imu_U;
    // the state packet went into x[0]: the candidate buffer and the solve's origin are copies
    int NS; const double* x0; double* x1; double* xorig;
};
// blocks [0, nbf): thread = visual factor; [nbf, nbf + n_imu): one IMU factor each; the rest: state copies
__global__ __launch_bounds__(256) void k_win_pack(WinPack A, int nbf) {
    const int t = threadIdx.x;
    int b = blockIdx.x;
    if (b < nbf) {
        const int f = b * 256 + t;
        if (f >= A.F) return;
        int lo = 0, hi = A.L - 1;                        // last landmark with lm_start[l] <= f
        while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (A.lm_start[mid] <= f) lo = mid; else hi = mid - 1; }
        const int l = lo, q = f - A.lm_start[l] + 1, s = A.lm_startf[l], ts = A.lm_track[l];
        const double* oi = A.store + ((size_t)A.fslot[s] * A.T + ts) * VIL_WIN_OBS;
        const double* oj = A.store + ((size_t)A.fslot[s + q] * A.T + ts) * VIL_WIN_OBS;
        const int fs = A.vfinv[f];                       // sorted position of this factor: the sweep's tables are stored in its chunk order
        double* c = A.vis_c + fs; const size_t st = (size_t)A.stride;
        // [0:3) pts_i  [3:6) pts_j  [6:8) vel_i  [8:10) vel_j  [10] td_i  [11] td_j  [12] row_i  [13] row_j   (vilsolve.h)
        c[0] = oi[0]; c[st] = oi[1]; c[2 * st] = oi[2]; c[3 * st] = oj[0]; c[4 * st] = oj[1]; c[5 * st] = oj[2];
        c[6 * st] = oi[3]; c[7 * st] = oi[4]; c[8 * st] = oj[3]; c[9 * st] = oj[4];
        c[10 * st] = oi[5]; c[11 * st] = oj[5]; c[12 * st] = oi[6]; c[13 * st] = oj[6];
        A.vis_i[fs] = s; A.vis_j[fs] = s + q; A.vis_l[fs] = l; A.fcol[f] = 6 * (s + q);
        return;
    }
    b -= nbf;
    if (b < A.n_imu) {
        const double* r = A.rec + (size_t)A.islot[b + 1] * 287; const double* u = A.U + (size_t)A.islot[b + 1] * 225;
        for (int e = t; e < 287; e += 256) A.imu_c[(size_t)b * 287 + e] = r[e];
        for (int e = t; e < 225; e += 256) A.imu_U[(size_t)b * 225 + e] = u[e];
        return;
    }
    b -= A.n_imu;
    const int nb = gridDim.x - nbf - A.n_imu;
    for (int e = b * 256 + t; e < A.NS; e += nb * 256) { const double v = A.x0[e]; A.x1[e] = v; A.xorig[e] = v; }
}
