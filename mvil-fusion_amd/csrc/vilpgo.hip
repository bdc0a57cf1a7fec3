// vilpgo.hip -- pose-graph optimisation on gfx950 behind include/vilpgo.h (the graph lidar_mapping keeps in GTSAM, globalMappingIkdTree.cpp:153-270, :379-508).
//
// The graph is resident: poses (two buffers: current and candidate), factor records, and per factor the whitened residual and Jacobians of both
// buffers.  vpgo_optimize enqueues the initial linearisation and then max_iterations times the same sequence; every kernel starts by reading the
// control block and returns at once when the device has finished (or, inside an attempt, when the factorisation has failed):
//   k_pgo_lin        a lane per factor: r, J_i, J_j and the cost term of the current (initial) or the candidate state.
//   k_pgo_gather     a lane per entry of a pose's 6 x 6 blocks: H_kk + lambda I, g_k and the chain block H_k,k+1, each the sum over the pose's
//                    factors in ascending factor index through the adjacency table.
//   k_pgo_segment    a wave per chain segment: block-tridiagonal Cholesky.  Lane c < 19 owns one column: 0-5 the next off-diagonal block, 6 the
//                    gradient, 7-12 / 13-18 the coupling to the left / right separator.  The 6 x 6 pivot block is factored by every lane; the
//                    columns meet in LDS once per key.  The segment's 12 x 12 Schur term and its right-hand side are accumulated key by key.
//   k_pgo_schur      a lane per entry of the dense reduced system (lower triangle, the right-hand side as its last row): separator blocks, chain
//                    blocks between neighbouring separators, loop blocks through the adjacency table, minus the segments' terms.  A gather.
//   k_pgo_chol       one launch per 16-wide tile column, a workgroup per tile row: left-looking; the tile's update L(I,:) L(K,:)^T runs on the fp64
//                    matrix cores (v_mfma_f64_16x16x4_f64, operand layout of vil_step.hpp), four waves share the columns and their partial tiles
//                    are added in wave order; the diagonal tile is updated and factored by every workgroup, then the tile's triangular solve.
//   k_pgo_dense_back one workgroup: L^T x = y, tile column by tile column.
//   k_pgo_seg_back   a lane per segment: back substitution along the chain from the separators' steps; a lane per separator copies its step.
//   k_pgo_update     a lane per pose: the candidate state, the pose's term of the predicted decrease and its largest step component.
//   k_pgo_reduce     a workgroup per block of 256 factors (cost) or poses (predicted decrease, step size), summed by one thread in order.
//   k_pgo_decide     one thread: the partials in order, the gain ratio, accept or reject, lambda, termination.
//   k_pgo_finish     a lane per pose: the accepted state goes to buffer 0.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/vilpgo.h"
#include "vil_host.hpp"
#include "vil_math.hpp"

#define PG_BLK VPGO_SUM_BLOCK
#define PG_NCOL 19                   // columns of a segment's working set
#define PG_NPAD_MAX (((6 * VPGO_MAX_SEPARATORS + 1 + 15) / 16) * 16)

namespace {

using vd::d4;

enum { K_LIN = 0, K_GATHER, K_SEGMENT, K_SCHUR, K_CHOL, K_DBACK, K_SBACK, K_UPDATE, K_REDUCE, K_DECIDE, K_FINISH };

struct PgFactor { int type, i, j, pad; double Z[12]; double sig[6]; };      // Z: rotation (9, row major) | translation (3); sig = sqrt(var)

struct PgCtl {                       // uploaded before a run, read back after it: the summary
    int done, bad, cur, iters, accepted, term, max_iter, pad;
    double lambda, nu, cost_cur, cost0, step_tol, cost_tol;
};

struct PgDev {                       // device pointers, by value in the kernel arguments
    PgCtl* ctl;
    double* X;                       // [2][max_poses][12]
    const PgFactor* fac;
    double* Rf; double* Ji; double* Jj; double* Cf;      // [2][max_factors][6 | 36 | 36 | 1]
    const int* adj_off; const int* adj;                  // per pose: entries 2 f + side in ascending f
    double* Hd; double* g; double* E;                    // per pose: 36 | 6 | 36
    const int* sep_key; const int* seg_a; const int* seg_b; const int* seg_l; const int* seg_r; const int* sep_segl; const int* sep_segr;
    double* Lk; double* Uk; double* Yk;                  // per pose: 21 | 36 | 13 x 6
    double* segM;                                        // per segment: 12 x 13
    double* A; double* Lm; double* xs;                   // dense reduced system, its factor, its solution
    double* delta; double* pred; double* maxd;           // per pose: 6 | 1 | 1
    double* part;                                        // partials: cost | pred | maxd
    int N, F, ns, nseg, n, ld, max_poses, max_factors, pstride;
};

__device__ __forceinline__ bool pg_idle(const PgCtl* c) { return c->done != 0; }
__device__ __forceinline__ bool pg_skip(const PgCtl* c) { return c->done != 0 || c->bad != 0; }

__device__ __forceinline__ void mat3_tmul(const double* A, const double* B, double* C) {      // C = A^T B
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) C[3 * r + c] = (A[r] * B[c] + A[3 + r] * B[3 + c]) + A[6 + r] * B[6 + c];
}
__device__ __forceinline__ void mat3_tvec(const double* A, const double* v, double* o) {      // o = A^T v
#pragma unroll
    for (int r = 0; r < 3; ++r) o[r] = (A[r] * v[0] + A[3 + r] * v[1]) + A[6 + r] * v[2];
}

// Log of the header, and Jri(Log)
__device__ __forceinline__ void so3_log_jri(const double* A, double* w, double* J) {
    const double v0 = 0.5 * (A[7] - A[5]), v1 = 0.5 * (A[2] - A[6]), v2 = 0.5 * (A[3] - A[1]);
    const double s = sqrt((v0 * v0 + v1 * v1) + v2 * v2), c = 0.5 * (((A[0] + A[4]) + A[8]) - 1.0);
    const double th = atan2(s, c), t2 = th * th;
    double k, e;
    if (th < VPGO_SMALL_ANGLE) { k = 1.0 + t2 / 6.0 + 7.0 * t2 * t2 / 360.0; e = 1.0 / 12.0 + t2 / 720.0; }
    else { k = th / s; e = 1.0 / t2 - (1.0 + cos(th)) / (2.0 * th * sin(th)); }
    w[0] = k * v0; w[1] = k * v1; w[2] = k * v2;
    const double ww = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
    J[0] = 1.0 + e * (w[0] * w[0] - ww); J[1] = -0.5 * w[2] + e * (w[0] * w[1]); J[2] = 0.5 * w[1] + e * (w[0] * w[2]);
    J[3] = 0.5 * w[2] + e * (w[1] * w[0]); J[4] = 1.0 + e * (w[1] * w[1] - ww); J[5] = -0.5 * w[0] + e * (w[1] * w[2]);
    J[6] = -0.5 * w[1] + e * (w[2] * w[0]); J[7] = 0.5 * w[0] + e * (w[2] * w[1]); J[8] = 1.0 + e * (w[2] * w[2] - ww);
}

__global__ __launch_bounds__(64) void k_pgo_lin(PgDev P, int sel) {
    if (pg_skip(P.ctl)) return;
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f >= P.F) return;
    const int b = sel ? 1 - P.ctl->cur : P.ctl->cur;
    const double* X = P.X + (size_t)b * P.max_poses * 12;
    const PgFactor* fc = P.fac + f;
    const int type = fc->type;
    const double* Xi = X + (size_t)fc->i * 12;
    double* r = P.Rf + ((size_t)b * P.max_factors + f) * 6;
    double* Ji = P.Ji + ((size_t)b * P.max_factors + f) * 36;
    double* Jj = P.Jj + ((size_t)b * P.max_factors + f) * 36;
    double is[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) is[q] = fc->sig[q];
    double wr[6];
#pragma unroll
    for (int q = 0; q < 36; ++q) { Ji[q] = 0.0; Jj[q] = 0.0; }
    if (type == VPGO_POSITION) {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const double v = (Xi[9 + q] - fc->Z[9 + q]) / is[q];
            r[q] = v; r[3 + q] = 0.0; wr[q] = v; wr[3 + q] = 0.0;
#pragma unroll
            for (int c = 0; c < 3; ++c) Ji[6 * q + 3 + c] = Xi[3 * q + c] / is[q];
        }
    } else {
        // a prior is the between factor from the identity: R_ij = R_i, p = t_i, and its Jacobian is the second pose's
        const bool btw = type == VPGO_BETWEEN;
        double* Jm = btw ? Jj : Ji;
        double Rij[9], p[3], d[3];
        if (btw) {
            const double* Xj = X + (size_t)fc->j * 12;
            double Ri[9], Rj[9];
#pragma unroll
            for (int q = 0; q < 9; ++q) { Ri[q] = Xi[q]; Rj[q] = Xj[q]; }
            mat3_tmul(Ri, Rj, Rij);
#pragma unroll
            for (int q = 0; q < 3; ++q) d[q] = Xj[9 + q] - Xi[9 + q];
            mat3_tvec(Ri, d, p);
        } else {
#pragma unroll
            for (int q = 0; q < 9; ++q) Rij[q] = Xi[q];
#pragma unroll
            for (int q = 0; q < 3; ++q) p[q] = Xi[9 + q];
        }
        double Zr[9];
#pragma unroll
        for (int q = 0; q < 9; ++q) Zr[q] = fc->Z[q];
        {
            double rt[3];
#pragma unroll
            for (int q = 0; q < 3; ++q) d[q] = p[q] - fc->Z[9 + q];
            mat3_tvec(Zr, d, rt);
#pragma unroll
            for (int q = 0; q < 3; ++q) { wr[3 + q] = rt[q] / is[3 + q]; r[3 + q] = wr[3 + q]; }
        }
        if (btw) {                                                      // rows 3-5 of J_i: [Z_R^T [p]x, -Z_R^T], [p]x = [0 -p2 p1; p2 0 -p0; -p1 p0 0]
            const double px[9] = {0.0, -p[2], p[1], p[2], 0.0, -p[0], -p[1], p[0], 0.0};
            double ZP[9];
            mat3_tmul(Zr, px, ZP);
#pragma unroll
            for (int q = 0; q < 3; ++q)
#pragma unroll
                for (int c = 0; c < 3; ++c) { Ji[6 * (3 + q) + c] = ZP[3 * q + c] / is[3 + q]; Ji[6 * (3 + q) + 3 + c] = -Zr[3 * c + q] / is[3 + q]; }
        }
        double A[9], w[3], Jr[9];
        mat3_tmul(Zr, Rij, A);
#pragma unroll
        for (int q = 0; q < 3; ++q)
#pragma unroll
            for (int c = 0; c < 3; ++c) Jm[6 * (3 + q) + 3 + c] = A[3 * q + c] / is[3 + q];
        so3_log_jri(A, w, Jr);
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            wr[q] = w[q] / is[q]; r[q] = wr[q];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                Jm[6 * q + c] = Jr[3 * q + c] / is[q];
                if (btw) Ji[6 * q + c] = -((Jr[3 * q] * Rij[3 * c] + Jr[3 * q + 1] * Rij[3 * c + 1]) + Jr[3 * q + 2] * Rij[3 * c + 2]) / is[q];      // -(Jri R_ij^T)
            }
        }
    }
    double cost = 0.0;
    {
#pragma clang fp contract(off)                                          // the cost's one order: six unfused squares added from 0.0
#pragma unroll
        for (int q = 0; q < 6; ++q) { const double sq = wr[q] * wr[q]; cost = cost + sq; }
    }
    P.Cf[(size_t)b * P.max_factors + f] = 0.5 * cost;
}

// thread = (pose, a, b): H[a][b], E[a][b]; the b == 0 lanes also g[a]
__global__ __launch_bounds__(256) void k_pgo_gather(PgDev P) {
    if (pg_idle(P.ctl)) return;
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int k = t / 36, e = t - 36 * k, a = e / 6, b = e - 6 * a;
    if (k >= P.N) return;
    const int cur = P.ctl->cur;
    const double lambda = P.ctl->lambda;
    const double* Rf = P.Rf + (size_t)cur * P.max_factors * 6;
    const double* Ji = P.Ji + (size_t)cur * P.max_factors * 36;
    const double* Jj = P.Jj + (size_t)cur * P.max_factors * 36;
    double H = 0.0, Ev = 0.0, gv = 0.0;
    for (int q = P.adj_off[k]; q < P.adj_off[k + 1]; ++q) {
        const int en = P.adj[q], f = en >> 1, side = en & 1;
        const double* J = (side ? Jj : Ji) + (size_t)f * 36;
        double c = 0.0, cg = 0.0;
#pragma unroll
        for (int r = 0; r < 6; ++r) { c += J[6 * r + a] * J[6 * r + b]; cg += J[6 * r + a] * Rf[(size_t)f * 6 + r]; }
        H = H + c; gv = gv + cg;
        const PgFactor* fc = P.fac + f;
        if (fc->type == VPGO_BETWEEN && (side ? fc->i : fc->j) == k + 1) {
            const double* Jo = (side ? Ji : Jj) + (size_t)f * 36;
            double ce = 0.0;
#pragma unroll
            for (int r = 0; r < 6; ++r) ce += J[6 * r + a] * Jo[6 * r + b];
            Ev = Ev + ce;
        }
    }
    P.Hd[(size_t)k * 36 + e] = (a == b) ? H + lambda : H;
    P.E[(size_t)k * 36 + e] = Ev;
    if (b == 0) P.g[(size_t)k * 6 + a] = gv;
}

// lower triangle index
#define LT(i, j) ((i) * ((i) + 1) / 2 + (j))

// in-register Cholesky of a 6 x 6 lower triangle (21 entries); false on a pivot that is not positive and finite
__device__ __forceinline__ bool chol6(double* L) {
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double d = L[LT(j, j)];
#pragma unroll
        for (int q = 0; q < j; ++q) d -= L[LT(j, q)] * L[LT(j, q)];
        ok = ok && d > 0.0 && isfinite(d);
        double sq, rs;
        vd::sqrt_rsqrt(d, sq, rs);
        L[LT(j, j)] = sq;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double v = L[LT(i, j)];
#pragma unroll
            for (int q = 0; q < j; ++q) v -= L[LT(i, q)] * L[LT(j, q)];
            L[LT(i, j)] = v / sq;
        }
    }
    return ok;
}

__global__ __launch_bounds__(64) void k_pgo_segment(PgDev P) {
    if (pg_idle(P.ctl)) return;
    __shared__ double Ush[36], Ysh[13 * 6], Msh[12 * 13];          // Msh: the segment's Schur terms, row = the lane's column
    const int seg = blockIdx.x, c = threadIdx.x;
    const int a = P.seg_a[seg], b = P.seg_b[seg];
    const bool hasL = P.seg_l[seg] >= 0, hasR = P.seg_r[seg] >= 0;
    double L[21], v[6];
    if (c >= 7 && c < PG_NCOL) {
#pragma unroll
        for (int q = 0; q < 13; ++q) Msh[13 * (c - 7) + q] = 0.0;
    }
    for (int k = a; k <= b; ++k) {
        const double* Hk = P.Hd + (size_t)k * 36;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) {
                double d = Hk[6 * i + j];
                if (k > a) {
#pragma unroll
                    for (int r = 0; r < 6; ++r) d -= Ush[6 * r + i] * Ush[6 * r + j];
                }
                L[LT(i, j)] = d;
            }
        if (!chol6(L)) { if (c == 0) P.ctl->bad = 1; return; }          // the same data in every lane: a uniform exit
        const double* Ek = P.E + (size_t)k * 36;
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            double x = 0.0;
            if (c < 6) x = (k < b) ? Ek[6 * r + c] : 0.0;
            else if (c == 6) x = P.g[(size_t)k * 6 + r];
            else if (c < 13) x = (k == a && hasL) ? P.E[(size_t)(a - 1) * 36 + 6 * (c - 7) + r] : 0.0;
            else if (c < PG_NCOL) x = (k == b && hasR) ? Ek[6 * r + (c - 13)] : 0.0;
            v[r] = x;
        }
        if (c >= 6 && c < PG_NCOL && k > a) {
#pragma unroll
            for (int p = 0; p < 6; ++p)
#pragma unroll
                for (int r = 0; r < 6; ++r) v[p] -= Ush[6 * r + p] * Ysh[6 * (c - 6) + r];      // the lane's own column at the previous key
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) {
#pragma unroll
            for (int q = 0; q < i; ++q) v[i] -= L[LT(i, q)] * v[q];
            v[i] = v[i] / L[LT(i, i)];
        }
        __syncthreads();                                                // everybody has read the previous key's U
        if (c < 6) {
#pragma unroll
            for (int r = 0; r < 6; ++r) { Ush[6 * r + c] = v[r]; P.Uk[(size_t)k * 36 + 6 * r + c] = v[r]; }
        } else if (c < PG_NCOL) {
#pragma unroll
            for (int r = 0; r < 6; ++r) { Ysh[6 * (c - 6) + r] = v[r]; P.Yk[(size_t)k * 78 + 6 * (c - 6) + r] = v[r]; }
        }
        if (c == 0) {
#pragma unroll
            for (int q = 0; q < 21; ++q) P.Lk[(size_t)k * 21 + q] = L[q];
        }
        __syncthreads();
        if (c >= 7 && c < PG_NCOL) {
#pragma unroll
            for (int q = 0; q < 13; ++q) {
                const double* y = Ysh + 6 * ((q < 12) ? q + 1 : 0);     // q < 12: coupling column q; 12: the gradient column
                double d = 0.0;
#pragma unroll
                for (int r = 0; r < 6; ++r) d += y[r] * v[r];
                Msh[13 * (c - 7) + q] = Msh[13 * (c - 7) + q] + d;
            }
        }
    }
    if (c >= 7 && c < PG_NCOL) {
#pragma unroll
        for (int q = 0; q < 13; ++q) P.segM[(size_t)seg * 156 + 13 * (c - 7) + q] = Msh[13 * (c - 7) + q];
    }
}

__global__ __launch_bounds__(256) void k_pgo_schur(PgDev P) {
    if (pg_skip(P.ctl)) return;
    const int ld = P.ld, n = P.n;
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)ld * ld) return;
    const int p = (int)(t / ld), q = (int)(t - (size_t)p * ld);
    double val = 0.0;
    if (q > p) { P.A[t] = 0.0; return; }
    if (p > n || q >= n) val = (p == q) ? 1.0 : 0.0;
    else if (p == n) {
        const int sq = q / 6, b = q - 6 * sq, kq = P.sep_key[sq];
        val = -P.g[(size_t)kq * 6 + b];
        const int sl = P.sep_segl[sq], sr = P.sep_segr[sq];
        if (sl >= 0) val += P.segM[(size_t)sl * 156 + 13 * (6 + b) + 12];
        if (sr >= 0) val += P.segM[(size_t)sr * 156 + 13 * b + 12];
    } else {
        const int sp = p / 6, a = p - 6 * sp, sq = q / 6, b = q - 6 * sq, kp = P.sep_key[sp], kq = P.sep_key[sq];
        if (sp == sq) {
            val = P.Hd[(size_t)kp * 36 + 6 * a + b];
            const int sl = P.sep_segl[sp], sr = P.sep_segr[sp];
            if (sl >= 0) val -= P.segM[(size_t)sl * 156 + 13 * (6 + b) + 6 + a];
            if (sr >= 0) val -= P.segM[(size_t)sr * 156 + 13 * b + a];
        } else {
            if (kp - kq == 1) val = P.E[(size_t)kq * 36 + 6 * b + a];
            else {
                const int cur = P.ctl->cur;
                const double* Ji = P.Ji + (size_t)cur * P.max_factors * 36;
                const double* Jj = P.Jj + (size_t)cur * P.max_factors * 36;
                for (int u = P.adj_off[kp]; u < P.adj_off[kp + 1]; ++u) {
                    const int en = P.adj[u], f = en >> 1, side = en & 1;
                    const PgFactor* fc = P.fac + f;
                    if (fc->type != VPGO_BETWEEN || (side ? fc->i : fc->j) != kq) continue;
                    const double* Jp = (side ? Jj : Ji) + (size_t)f * 36; const double* Jq = (side ? Ji : Jj) + (size_t)f * 36;
                    double c = 0.0;
#pragma unroll
                    for (int r = 0; r < 6; ++r) c += Jp[6 * r + a] * Jq[6 * r + b];
                    val = val + c;
                }
            }
            const int sg = P.sep_segl[sp];
            if (sq == sp - 1 && sg >= 0 && P.sep_segr[sq] == sg) val -= P.segM[(size_t)sg * 156 + 13 * b + 6 + a];
        }
    }
    P.A[t] = val;
}

// tile column Kt of the factor; workgroup blockIdx.x owns tile row I = Kt + blockIdx.x.  Operand lane layout as vil_step.hpp: A / B fragment
// (row lane & 15, k lane >> 4), accumulator (row (lane >> 4) + 4 g, column lane & 15).
__global__ __launch_bounds__(256) void k_pgo_chol(PgDev P, int Kt) {
    if (pg_skip(P.ctl)) return;
    __shared__ double part[4][2][256];
    __shared__ double Td[16 * 17], To[16 * 17];
    __shared__ int s_bad;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, I = Kt + blockIdx.x, ld = P.ld, n = P.n;
    const double* Lm = P.Lm;
    d4 accO = {0.0, 0.0, 0.0, 0.0}, accD = {0.0, 0.0, 0.0, 0.0};
    const size_t ro = (size_t)(16 * I + (lane & 15)) * ld + (lane >> 4), rd = (size_t)(16 * Kt + (lane & 15)) * ld + (lane >> 4);
    for (int J = wave; J < Kt; J += 4) {
#pragma unroll
        for (int ks = 0; ks < 16; ks += 4) {
            const double av = Lm[ro + 16 * J + ks], bv = Lm[rd + 16 * J + ks];
            accO = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, accO, 0, 0, 0);
            accD = __builtin_amdgcn_mfma_f64_16x16x4f64(bv, bv, accD, 0, 0, 0);
        }
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int e = ((lane >> 4) + 4 * g) * 16 + (lane & 15);
        part[wave][0][e] = accO[g]; part[wave][1][e] = accD[g];
    }
    if (t == 0) s_bad = 0;
    __syncthreads();
    const int r = t >> 4, c = t & 15;
    To[r * 17 + c] = P.A[(size_t)(16 * I + r) * ld + 16 * Kt + c] - (((part[0][0][t] + part[1][0][t]) + part[2][0][t]) + part[3][0][t]);
    Td[r * 17 + c] = P.A[(size_t)(16 * Kt + r) * ld + 16 * Kt + c] - (((part[0][1][t] + part[1][1][t]) + part[2][1][t]) + part[3][1][t]);
    __syncthreads();
    for (int k = 0; k < 16; ++k) {                                      // the diagonal tile, a row per thread of the first sixteen
        const bool live = 16 * Kt + k < n;                              // columns from the right-hand-side row on: unit pivot, nothing below
        double v = 0.0;
        if (t < 16 && t >= k) {
            v = Td[t * 17 + k];
            for (int j = 0; j < k; ++j) v -= Td[t * 17 + j] * Td[k * 17 + j];
        }
        if (t == k) {
            if (!live) v = 1.0;
            if (!(v > 0.0) || !isfinite(v)) { s_bad = 1; v = 1.0; }
            Td[k * 17 + k] = sqrt(v);
        }
        __syncthreads();
        if (t < 16 && t > k) Td[t * 17 + k] = live ? v / Td[k * 17 + k] : 0.0;
        __syncthreads();
    }
    if (I > Kt && t < 16) {                                             // X L^T = tile: a row per thread
        for (int k = 0; k < 16; ++k) {
            double v = To[t * 17 + k];
            for (int j = 0; j < k; ++j) v -= To[t * 17 + j] * Td[k * 17 + j];
            To[t * 17 + k] = (16 * Kt + k < n) ? v / Td[k * 17 + k] : 0.0;
        }
    }
    __syncthreads();
    P.Lm[(size_t)(16 * I + r) * ld + 16 * Kt + c] = (I > Kt) ? To[r * 17 + c] : (c <= r ? Td[r * 17 + c] : 0.0);
    if (t == 0 && s_bad) P.ctl->bad = 1;
}

__global__ __launch_bounds__(512) void k_pgo_dense_back(PgDev P) {
    if (pg_skip(P.ctl)) return;
    __shared__ double x[PG_NPAD_MAX];
    __shared__ double Td[16 * 17];
    const int t = threadIdx.x, n = P.n, ld = P.ld, Tn = (n + 15) >> 4;
    for (int j = t; j < 16 * Tn; j += 512) x[j] = j < n ? P.Lm[(size_t)n * ld + j] : 0.0;
    for (int K = Tn - 1; K >= 0; --K) {
        __syncthreads();
        if (t < 256) { const int r = t >> 4, c = t & 15; Td[r * 17 + c] = P.Lm[(size_t)(16 * K + r) * ld + 16 * K + c]; }
        __syncthreads();
        if (t == 0) {
            const int m = min(16, n - 16 * K);
            for (int k = m - 1; k >= 0; --k) {
                double v = x[16 * K + k];
                for (int r2 = k + 1; r2 < m; ++r2) v -= Td[r2 * 17 + k] * x[16 * K + r2];
                x[16 * K + k] = v / Td[k * 17 + k];
            }
        }
        __syncthreads();
        const int m = min(16, n - 16 * K);
        for (int j = t; j < 16 * K; j += 512) {
            double v = x[j];
            for (int r2 = 0; r2 < m; ++r2) v -= P.Lm[(size_t)(16 * K + r2) * ld + j] * x[16 * K + r2];
            x[j] = v;
        }
    }
    __syncthreads();
    for (int j = t; j < n; j += 512) P.xs[j] = x[j];
}

__global__ __launch_bounds__(64) void k_pgo_seg_back(PgDev P) {
    if (pg_skip(P.ctl)) return;
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= P.nseg + P.ns) return;
    if (t >= P.nseg) {
        const int s = t - P.nseg, k = P.sep_key[s];
#pragma unroll
        for (int q = 0; q < 6; ++q) P.delta[(size_t)k * 6 + q] = P.xs[6 * s + q];
        return;
    }
    const int a = P.seg_a[t], b = P.seg_b[t], sl = P.seg_l[t], sr = P.seg_r[t];
    double dl[6], dr[6], dn[6], d[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) { dl[q] = sl >= 0 ? P.xs[6 * sl + q] : 0.0; dr[q] = sr >= 0 ? P.xs[6 * sr + q] : 0.0; dn[q] = 0.0; }
    for (int k = b; k >= a; --k) {
        const double* Y = P.Yk + (size_t)k * 78; const double* U = P.Uk + (size_t)k * 36; const double* L = P.Lk + (size_t)k * 21;
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            double v = Y[r];
#pragma unroll
            for (int cc = 0; cc < 6; ++cc) v += Y[6 * (1 + cc) + r] * dl[cc];
#pragma unroll
            for (int cc = 0; cc < 6; ++cc) v += Y[6 * (7 + cc) + r] * dr[cc];
            v = -v;
            if (k < b) {
#pragma unroll
                for (int q = 0; q < 6; ++q) v -= U[6 * r + q] * dn[q];
            }
            d[r] = v;
        }
#pragma unroll
        for (int i = 5; i >= 0; --i) {                                  // L^T d = rhs
#pragma unroll
            for (int q = i + 1; q < 6; ++q) d[i] -= L[LT(q, i)] * d[q];
            d[i] = d[i] / L[LT(i, i)];
        }
#pragma unroll
        for (int q = 0; q < 6; ++q) { P.delta[(size_t)k * 6 + q] = d[q]; dn[q] = d[q]; }
    }
}

__global__ __launch_bounds__(64) void k_pgo_update(PgDev P) {
    if (pg_skip(P.ctl)) return;
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= P.N) return;
    const int cur = P.ctl->cur;
    const double lambda = P.ctl->lambda;
    const double* Xc = P.X + ((size_t)cur * P.max_poses + k) * 12;
    double* Xn = P.X + ((size_t)(1 - cur) * P.max_poses + k) * 12;
    double d[6], R[9];
    double pred = 0.0, md = 0.0;
#pragma unroll
    for (int q = 0; q < 6; ++q) { d[q] = P.delta[(size_t)k * 6 + q]; pred += d[q] * (lambda * d[q] - P.g[(size_t)k * 6 + q]); md = fmax(md, fabs(d[q])); }
#pragma unroll
    for (int q = 0; q < 9; ++q) R[q] = Xc[q];
#pragma unroll
    for (int r = 0; r < 3; ++r) Xn[9 + r] = Xc[9 + r] + ((R[3 * r] * d[3] + R[3 * r + 1] * d[4]) + R[3 * r + 2] * d[5]);
    const double t2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2], th = sqrt(t2);
    double ca, cb;
    if (th < VPGO_SMALL_ANGLE) { ca = 1.0 - t2 / 6.0; cb = 0.5 - t2 / 24.0; }
    else { const double sh = sin(0.5 * th); ca = sin(th) / th; cb = 2.0 * sh * sh / t2; }
    double Ex[9];
    Ex[0] = 1.0 + cb * (d[0] * d[0] - t2); Ex[1] = -ca * d[2] + cb * (d[0] * d[1]); Ex[2] = ca * d[1] + cb * (d[0] * d[2]);
    Ex[3] = ca * d[2] + cb * (d[1] * d[0]); Ex[4] = 1.0 + cb * (d[1] * d[1] - t2); Ex[5] = -ca * d[0] + cb * (d[1] * d[2]);
    Ex[6] = -ca * d[1] + cb * (d[2] * d[0]); Ex[7] = ca * d[0] + cb * (d[2] * d[1]); Ex[8] = 1.0 + cb * (d[2] * d[2] - t2);
    double M[9], G[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) M[3 * r + c] = (R[3 * r] * Ex[c] + R[3 * r + 1] * Ex[3 + c]) + R[3 * r + 2] * Ex[6 + c];
    mat3_tmul(M, M, G);
#pragma unroll
    for (int q = 0; q < 9; ++q) G[q] = ((q % 4 == 0) ? 3.0 : 0.0) - G[q];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) Xn[3 * r + c] = 0.5 * ((M[3 * r] * G[c] + M[3 * r + 1] * G[3 + c]) + M[3 * r + 2] * G[6 + c]);
    P.pred[k] = pred; P.maxd[k] = md;
}

// blocks [0, nfb): cost partials of buffer (sel ? candidate : current); blocks [nfb, nfb + npb): predicted decrease and step size
__global__ __launch_bounds__(PG_BLK) void k_pgo_reduce(PgDev P, int sel, int nfb) {
    if (pg_skip(P.ctl)) return;
    __shared__ double s_a[PG_BLK], s_b[PG_BLK];
    const int t = threadIdx.x, blk = blockIdx.x;
    if (blk < nfb) {
        const int b = sel ? 1 - P.ctl->cur : P.ctl->cur, f = blk * PG_BLK + t;
        s_a[t] = f < P.F ? P.Cf[(size_t)b * P.max_factors + f] : 0.0;
        __syncthreads();
        if (t == 0) {
            double acc = 0.0;
#pragma unroll 16
            for (int j = 0; j < PG_BLK; ++j) acc = acc + s_a[j];        // + 0.0 changes no bit of a sum >= 0
            P.part[blk] = acc;
        }
    } else {
        const int pb = blk - nfb, k = pb * PG_BLK + t;
        s_a[t] = k < P.N ? P.pred[k] : 0.0; s_b[t] = k < P.N ? P.maxd[k] : 0.0;
        __syncthreads();
        if (t == 0) {
            double acc = 0.0, mx = 0.0;
            const int m = min(PG_BLK, P.N - pb * PG_BLK);
            for (int j = 0; j < m; ++j) { acc = acc + s_a[j]; mx = fmax(mx, s_b[j]); }
            P.part[P.pstride + pb] = acc; P.part[2 * P.pstride + pb] = mx;
        }
    }
}

__global__ __launch_bounds__(64) void k_pgo_decide(PgDev P, int mode, int nfb, int npb) {
    PgCtl* c = P.ctl;
    if (threadIdx.x != 0 || c->done) return;
    double cost = 0.0;
    const bool bad = c->bad != 0;
    if (!bad) for (int j = 0; j < nfb; ++j) cost = cost + P.part[j];
    if (mode == 0) { c->cost_cur = cost; c->cost0 = cost; return; }
    double pred = 0.0, maxd = 0.0;
    if (!bad) for (int j = 0; j < npb; ++j) { pred = pred + P.part[P.pstride + j]; maxd = fmax(maxd, P.part[2 * P.pstride + j]); }
    pred = 0.5 * pred;
    c->iters += 1;
    const double dec = c->cost_cur - cost, rho = dec / pred;
    if (!bad && isfinite(cost) && pred > 0.0 && rho > 0.0) {
        const double rel = dec / c->cost_cur, u = 2.0 * rho - 1.0;
        c->cur ^= 1; c->cost_cur = cost; c->accepted += 1;
        c->lambda = c->lambda * fmax(1.0 / 3.0, 1.0 - u * u * u); c->nu = 2.0;
        if (maxd < c->step_tol) { c->done = 1; c->term = VPGO_TERM_STEP; }
        else if (rel < c->cost_tol) { c->done = 1; c->term = VPGO_TERM_COST; }
    } else {
        c->lambda = fmax(c->lambda * c->nu, VPGO_LAMBDA_FLOOR); c->nu = 2.0 * c->nu;
        if (!bad && maxd < c->step_tol) { c->done = 1; c->term = VPGO_TERM_STEP; }
    }
    c->bad = 0;
    if (!c->done && c->iters >= c->max_iter) { c->done = 1; c->term = VPGO_TERM_MAX_ITERATIONS; }
}

__global__ __launch_bounds__(64) void k_pgo_finish(PgDev P) {
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= P.N || P.ctl->cur == 0) return;
    const double* s = P.X + ((size_t)P.max_poses + k) * 12; double* d = P.X + (size_t)k * 12;
#pragma unroll
    for (int q = 0; q < 12; ++q) d[q] = s[q];
}

}  // namespace

struct vpgo_ctx : vilhost::Device {
    int max_poses = 0, max_factors = 0, N = 0, F = 0, ns = 0, nseg = 0, pstride = 0;
    bool dirty = true;                                       // the index tables on the device are older than the graph
    std::vector<int> f_type, f_i, f_j;                       // host mirror of the structure
    std::vector<char> is_sep;
    PgDev P{};
    char* h_stage = nullptr; int* h_idx = nullptr; PgCtl* h_ctl = nullptr;      // pinned: a record or poses | the index tables | the control block
    size_t o_idx = 0, idx_bytes = 0;
    size_t io_adj_off = 0, io_adj = 0, io_sep_key = 0, io_seg_a = 0, io_seg_b = 0, io_seg_l = 0, io_seg_r = 0, io_sep_segl = 0, io_sep_segr = 0;
    vilhost::EventLog<VPGO_NUM_KERNELS> prof;               // an event before every group of launches of one kernel
};

namespace {

bool finite_n(const double* v, int n) { for (int q = 0; q < n; ++q) if (!std::isfinite(v[q])) return false; return true; }
bool var_ok(const double* v, int n) { for (int q = 0; q < n; ++q) if (!(std::isfinite(v[q]) && v[q] > 0.0)) return false; return true; }

int upload_small(vpgo_ctx* c, void* dst, const void* src, size_t bytes) {
    VILCHK(hipSetDevice(c->device));
    memcpy(c->h_stage, src, bytes);
    VILCHK(hipMemcpyAsync(dst, c->h_stage, bytes, hipMemcpyHostToDevice, c->stream));
    VILCHK(hipStreamSynchronize(c->stream));
    return VIL_OK;
}

int add_factor(vpgo_ctx* c, int type, int i, int j, const double* Z12, const double* var, int nvar) {
    if (c->F >= c->max_factors) return VIL_ERR_CAPACITY;
    int fresh = 0;
    if (type == VPGO_BETWEEN && std::abs(i - j) > 1) {
        fresh = (c->is_sep[i] ? 0 : 1) + (c->is_sep[j] ? 0 : 1);
        if (c->ns + fresh > VPGO_MAX_SEPARATORS) return VIL_ERR_CAPACITY;
    }
    PgFactor f;
    memset(&f, 0, sizeof f);
    f.type = type; f.i = i; f.j = j;
    for (int q = 0; q < 12; ++q) f.Z[q] = Z12[q];
    for (int q = 0; q < 6; ++q) f.sig[q] = q < nvar ? std::sqrt(var[q]) : 1.0;
    const int st = upload_small(c, (void*)(c->P.fac + c->F), &f, sizeof f);
    if (st != VIL_OK) return st;
    if (fresh) { c->is_sep[i] = 1; c->is_sep[j] = 1; c->ns += fresh; }
    c->f_type.push_back(type); c->f_i.push_back(i); c->f_j.push_back(j);
    c->F += 1; c->dirty = true;
    return VIL_OK;
}

void rows12(const double* T16, double* o) {                 // 4 x 4 row major -> rotation (9) | translation (3)
    for (int r = 0; r < 3; ++r) { for (int q = 0; q < 3; ++q) o[3 * r + q] = T16[4 * r + q]; o[9 + r] = T16[4 * r + 3]; }
}
void mat16(const double* x, double* T) {
    for (int r = 0; r < 3; ++r) { for (int q = 0; q < 3; ++q) T[4 * r + q] = x[3 * r + q]; T[4 * r + 3] = x[9 + r]; }
    T[12] = T[13] = T[14] = 0.0; T[15] = 1.0;
}

// adjacency, separators and segments from the host mirror; one upload
int sync_tables(vpgo_ctx* c) {
    if (!c->dirty) return VIL_OK;
    const int N = c->N, F = c->F;
    int* h = c->h_idx;
    int* adj_off = h + c->io_adj_off; int* adj = h + c->io_adj; int* sep_key = h + c->io_sep_key;
    int* seg_a = h + c->io_seg_a; int* seg_b = h + c->io_seg_b; int* seg_l = h + c->io_seg_l; int* seg_r = h + c->io_seg_r;
    int* sep_segl = h + c->io_sep_segl; int* sep_segr = h + c->io_sep_segr;
    for (int k = 0; k <= N; ++k) adj_off[k] = 0;
    for (int f = 0; f < F; ++f) { adj_off[c->f_i[f] + 1]++; if (c->f_type[f] == VPGO_BETWEEN) adj_off[c->f_j[f] + 1]++; }
    for (int k = 0; k < N; ++k) adj_off[k + 1] += adj_off[k];
    std::vector<int> fill(adj_off, adj_off + N);
    for (int f = 0; f < F; ++f) { adj[fill[c->f_i[f]]++] = 2 * f; if (c->f_type[f] == VPGO_BETWEEN) adj[fill[c->f_j[f]]++] = 2 * f + 1; }
    int ns = 0, nseg = 0, last_sep = -1, start = 0;
    for (int k = 0; k <= N; ++k) {
        const bool sep = k < N && c->is_sep[k];
        if (sep || k == N) {
            if (k > start) { seg_a[nseg] = start; seg_b[nseg] = k - 1; seg_l[nseg] = last_sep; seg_r[nseg] = sep ? ns : -1; if (last_sep >= 0) sep_segr[last_sep] = nseg; if (sep) sep_segl[ns] = nseg; ++nseg; }
            else if (sep) sep_segl[ns] = -1;
            if (sep) { sep_key[ns] = k; sep_segr[ns] = -1; last_sep = ns; ++ns; }
            start = k + 1;
        }
    }
    c->nseg = nseg;
    VILCHK(hipSetDevice(c->device));
    VILCHK(hipMemcpyAsync(c->d_mem + c->o_idx, h, c->idx_bytes, hipMemcpyHostToDevice, c->stream));
    VILCHK(hipStreamSynchronize(c->stream));
    c->dirty = false;
    return VIL_OK;
}

PgDev params(vpgo_ctx* c) {
    PgDev P = c->P;
    P.N = c->N; P.F = c->F; P.ns = c->ns; P.nseg = c->nseg; P.n = 6 * c->ns; P.ld = ((6 * c->ns + 1 + 15) / 16) * 16;
    return P;
}

int put_ctl(vpgo_ctx* c, const vpgo_options* o) {
    PgCtl k;
    memset(&k, 0, sizeof k);
    k.max_iter = o ? o->max_iterations : 0; k.lambda = o ? o->initial_lambda : 0.0; k.nu = 2.0;
    k.step_tol = o ? o->step_tolerance : 0.0; k.cost_tol = o ? o->cost_tolerance : 0.0;
    *c->h_ctl = k;
    VILCHK(hipMemcpyAsync(c->P.ctl, c->h_ctl, sizeof k, hipMemcpyHostToDevice, c->stream));
    return VIL_OK;
}

}  // namespace

extern "C" {

int vpgo_create(int32_t device, int32_t max_poses, int32_t max_factors, vpgo_ctx** out) {
    if (!out || max_poses <= 0 || max_factors <= 0) return VIL_ERR_INVALID_ARGUMENT;
    vpgo_ctx* c = new vpgo_ctx();
    c->max_poses = max_poses; c->max_factors = max_factors;
    const size_t N = (size_t)max_poses, F = (size_t)max_factors, S = VPGO_MAX_SEPARATORS, G = S + 1, ld = PG_NPAD_MAX;
    c->pstride = (int)((std::max(N, F) + PG_BLK - 1) / PG_BLK);
    vilhost::Arena a;
    const size_t o_ctl = a.take(sizeof(PgCtl)), o_X = a.take(8 * 2 * N * 12), o_fac = a.take(sizeof(PgFactor) * F);
    const size_t o_Rf = a.take(8 * 2 * F * 6), o_Ji = a.take(8 * 2 * F * 36), o_Jj = a.take(8 * 2 * F * 36), o_Cf = a.take(8 * 2 * F);
    const size_t o_Hd = a.take(8 * N * 36), o_g = a.take(8 * N * 6), o_E = a.take(8 * N * 36);
    const size_t o_Lk = a.take(8 * N * 21), o_Uk = a.take(8 * N * 36), o_Yk = a.take(8 * N * 78), o_segM = a.take(8 * G * 156);
    const size_t o_A = a.take(8 * ld * ld), o_Lm = a.take(8 * ld * ld), o_xs = a.take(8 * ld);
    const size_t o_delta = a.take(8 * N * 6), o_pred = a.take(8 * N), o_maxd = a.take(8 * N), o_part = a.take(8 * 3 * (size_t)c->pstride);
    // the index tables: one block, uploaded together
    size_t ni = 0;
    auto take_i = [&](size_t n) { const size_t o = ni; ni += (n + 3) & ~(size_t)3; return o; };
    c->io_adj_off = take_i(N + 1); c->io_adj = take_i(2 * F); c->io_sep_key = take_i(S);
    c->io_seg_a = take_i(G); c->io_seg_b = take_i(G); c->io_seg_l = take_i(G); c->io_seg_r = take_i(G); c->io_sep_segl = take_i(S); c->io_sep_segr = take_i(S);
    c->idx_bytes = 4 * ni;
    c->o_idx = a.take(c->idx_bytes);
    hipError_t err = c->open(device, a.bytes);
    if (err == hipSuccess) err = c->pin(&c->h_stage, std::max(sizeof(PgFactor), 8 * N * 12));
    if (err == hipSuccess) err = c->pin(&c->h_idx, c->idx_bytes);
    if (err == hipSuccess) err = c->pin(&c->h_ctl, sizeof(PgCtl));
    if (err != hipSuccess) { vpgo_destroy(c); VILCHK(err); }
    char* d = c->d_mem;
    PgDev& P = c->P;
    P.ctl = (PgCtl*)(d + o_ctl); P.X = (double*)(d + o_X); P.fac = (const PgFactor*)(d + o_fac);
    P.Rf = (double*)(d + o_Rf); P.Ji = (double*)(d + o_Ji); P.Jj = (double*)(d + o_Jj); P.Cf = (double*)(d + o_Cf);
    P.Hd = (double*)(d + o_Hd); P.g = (double*)(d + o_g); P.E = (double*)(d + o_E);
    P.Lk = (double*)(d + o_Lk); P.Uk = (double*)(d + o_Uk); P.Yk = (double*)(d + o_Yk); P.segM = (double*)(d + o_segM);
    P.A = (double*)(d + o_A); P.Lm = (double*)(d + o_Lm); P.xs = (double*)(d + o_xs);
    P.delta = (double*)(d + o_delta); P.pred = (double*)(d + o_pred); P.maxd = (double*)(d + o_maxd); P.part = (double*)(d + o_part);
    const int* di = (const int*)(d + c->o_idx);
    P.adj_off = di + c->io_adj_off; P.adj = di + c->io_adj; P.sep_key = di + c->io_sep_key;
    P.seg_a = di + c->io_seg_a; P.seg_b = di + c->io_seg_b; P.seg_l = di + c->io_seg_l; P.seg_r = di + c->io_seg_r;
    P.sep_segl = di + c->io_sep_segl; P.sep_segr = di + c->io_sep_segr;
    P.max_poses = max_poses; P.max_factors = max_factors; P.pstride = c->pstride;
    c->is_sep.assign(N, 0);
    *out = c;
    return VIL_OK;
}

void vpgo_destroy(vpgo_ctx* c) {
    if (!c) return;
    c->close(c->prof);
    delete c;
}

void vpgo_default_options(vpgo_options* o) {
    if (!o) return;
    o->max_iterations = 20; o->pad = 0; o->initial_lambda = 1e-5; o->step_tolerance = 1e-10; o->cost_tolerance = 1e-12;
}

int vpgo_profile_enable(vpgo_ctx* c, int32_t enable) {
    if (!c) return VIL_ERR_INVALID_ARGUMENT;
    c->prof.on = enable != 0;
    return VIL_OK;
}
int vpgo_profile_read(vpgo_ctx* c, int64_t* launches, double* total_ms) {
    if (!c || !launches || !total_ms) return VIL_ERR_INVALID_ARGUMENT;
    c->prof.read(launches, total_ms);
    return VIL_OK;
}

int vpgo_size(vpgo_ctx* c, int32_t* n_poses, int32_t* n_factors, int32_t* n_separators) {
    if (!c) return VIL_ERR_INVALID_ARGUMENT;
    if (n_poses) *n_poses = c->N;
    if (n_factors) *n_factors = c->F;
    if (n_separators) *n_separators = c->ns;
    return VIL_OK;
}

int vpgo_add_pose(vpgo_ctx* c, const double* T16, int32_t* key) {
    if (!c || !T16) return VIL_ERR_INVALID_ARGUMENT;
    if (!finite_n(T16, 16)) return VIL_ERR_NON_FINITE;
    if (c->N >= c->max_poses) return VIL_ERR_CAPACITY;
    const bool sep = (c->N + 1) % VPGO_SEGMENT == 0;
    if (sep && c->ns + 1 > VPGO_MAX_SEPARATORS) return VIL_ERR_CAPACITY;
    double x[12];
    rows12(T16, x);
    const int st = upload_small(c, c->P.X + (size_t)c->N * 12, x, sizeof x);
    if (st != VIL_OK) return st;
    if (sep) { c->is_sep[c->N] = 1; c->ns += 1; }
    if (key) *key = c->N;
    c->N += 1; c->dirty = true;
    return VIL_OK;
}

int vpgo_add_prior(vpgo_ctx* c, int32_t i, const double* Z16, const double* var6) {
    if (!c || !Z16 || !var6 || i < 0 || i >= c->N) return VIL_ERR_INVALID_ARGUMENT;
    if (!finite_n(Z16, 16)) return VIL_ERR_NON_FINITE;
    if (!var_ok(var6, 6)) return VIL_ERR_INVALID_ARGUMENT;
    double z[12];
    rows12(Z16, z);
    return add_factor(c, VPGO_PRIOR, i, i, z, var6, 6);
}

int vpgo_add_between(vpgo_ctx* c, int32_t i, int32_t j, const double* Z16, const double* var6) {
    if (!c || !Z16 || !var6 || i < 0 || i >= c->N || j < 0 || j >= c->N || i == j) return VIL_ERR_INVALID_ARGUMENT;
    if (!finite_n(Z16, 16)) return VIL_ERR_NON_FINITE;
    if (!var_ok(var6, 6)) return VIL_ERR_INVALID_ARGUMENT;
    double z[12];
    rows12(Z16, z);
    return add_factor(c, VPGO_BETWEEN, i, j, z, var6, 6);
}

int vpgo_add_position(vpgo_ctx* c, int32_t i, const double* z3, const double* var3) {
    if (!c || !z3 || !var3 || i < 0 || i >= c->N) return VIL_ERR_INVALID_ARGUMENT;
    if (!finite_n(z3, 3)) return VIL_ERR_NON_FINITE;
    if (!var_ok(var3, 3)) return VIL_ERR_INVALID_ARGUMENT;
    double z[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, z3[0], z3[1], z3[2]};
    return add_factor(c, VPGO_POSITION, i, i, z, var3, 3);
}

int vpgo_get_poses(vpgo_ctx* c, int32_t first, int32_t n, double* T16s) {
    if (!c || !T16s || first < 0 || n < 0 || first > c->N - n) return VIL_ERR_INVALID_ARGUMENT;
    if (!n) return VIL_OK;
    VILCHK(hipSetDevice(c->device));
    VILCHK(hipMemcpyAsync(c->h_stage, c->P.X + (size_t)first * 12, 96 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    VILCHK(hipStreamSynchronize(c->stream));
    for (int k = 0; k < n; ++k) mat16((const double*)c->h_stage + 12 * (size_t)k, T16s + 16 * (size_t)k);
    return VIL_OK;
}

int vpgo_relative(vpgo_ctx* c, int32_t i, int32_t j, double* T16) {
    if (!c || !T16 || i < 0 || i >= c->N || j < 0 || j >= c->N) return VIL_ERR_INVALID_ARGUMENT;
    double Ti[16], Tj[16];
    int st = vpgo_get_poses(c, i, 1, Ti);
    if (st == VIL_OK) st = vpgo_get_poses(c, j, 1, Tj);
    if (st != VIL_OK) return st;
    for (int r = 0; r < 3; ++r) {                           // R_j^T R_i, R_j^T (t_i - t_j)
        for (int q = 0; q < 3; ++q) T16[4 * r + q] = (Tj[r] * Ti[q] + Tj[4 + r] * Ti[4 + q]) + Tj[8 + r] * Ti[8 + q];
        T16[4 * r + 3] = (Tj[r] * (Ti[3] - Tj[3]) + Tj[4 + r] * (Ti[7] - Tj[7])) + Tj[8 + r] * (Ti[11] - Tj[11]);
    }
    T16[12] = T16[13] = T16[14] = 0.0; T16[15] = 1.0;
    return VIL_OK;
}

int vpgo_get_step(vpgo_ctx* c, double* d) {
    if (!c || !d) return VIL_ERR_INVALID_ARGUMENT;
    if (!c->N) return VIL_OK;
    VILCHK(hipSetDevice(c->device));
    VILCHK(hipMemcpyAsync(c->h_stage, c->P.delta, 48 * (size_t)c->N, hipMemcpyDeviceToHost, c->stream));
    VILCHK(hipStreamSynchronize(c->stream));
    memcpy(d, c->h_stage, 48 * (size_t)c->N);
    return VIL_OK;
}

int vpgo_eval(vpgo_ctx* c, double* r, double* J_i, double* J_j, double* cost, double* g) {
    if (!c) return VIL_ERR_INVALID_ARGUMENT;
    VILCHK(hipSetDevice(c->device));
    int st = sync_tables(c);
    if (st != VIL_OK) return st;
    const PgDev P = params(c);
    const int N = c->N, F = c->F, nfb = (F + PG_BLK - 1) / PG_BLK;
    if ((st = put_ctl(c, nullptr)) != VIL_OK) return st;
    if (F) {
        hipLaunchKernelGGL(k_pgo_lin, dim3((F + 63) / 64), dim3(64), 0, c->stream, P, 0);
        hipLaunchKernelGGL(k_pgo_reduce, dim3(nfb), dim3(PG_BLK), 0, c->stream, P, 0, nfb);
    }
    if (N) hipLaunchKernelGGL(k_pgo_gather, dim3((36 * N + 255) / 256), dim3(256), 0, c->stream, P);
    hipLaunchKernelGGL(k_pgo_decide, dim3(1), dim3(64), 0, c->stream, P, 0, F ? nfb : 0, 0);
    VILCHK(hipMemcpyAsync(c->h_ctl, P.ctl, sizeof(PgCtl), hipMemcpyDeviceToHost, c->stream));
    if (r && F) VILCHK(hipMemcpyAsync(r, P.Rf, 48 * (size_t)F, hipMemcpyDeviceToHost, c->stream));
    if (J_i && F) VILCHK(hipMemcpyAsync(J_i, P.Ji, 288 * (size_t)F, hipMemcpyDeviceToHost, c->stream));
    if (J_j && F) VILCHK(hipMemcpyAsync(J_j, P.Jj, 288 * (size_t)F, hipMemcpyDeviceToHost, c->stream));
    if (g && N) VILCHK(hipMemcpyAsync(g, P.g, 48 * (size_t)N, hipMemcpyDeviceToHost, c->stream));
    VILCHK(hipStreamSynchronize(c->stream));
    VILCHK(hipGetLastError());
    if (cost) *cost = c->h_ctl->cost_cur;
    return VIL_OK;
}

int vpgo_optimize(vpgo_ctx* c, const vpgo_options* o, vpgo_summary* sm) {
    if (!c || !o || !sm || o->max_iterations < 1 || o->max_iterations > VPGO_MAX_ITERATIONS || !(o->initial_lambda >= 0.0) || !std::isfinite(o->initial_lambda) ||
        !(o->step_tolerance >= 0.0) || !(o->cost_tolerance >= 0.0))
        return VIL_ERR_INVALID_ARGUMENT;
    memset(sm, 0, sizeof *sm);
    VILCHK(hipSetDevice(c->device));
    int st = sync_tables(c);
    if (st != VIL_OK) return st;
    const PgDev P = params(c);
    const int N = c->N, F = c->F, ns = c->ns, nseg = c->nseg;
    sm->n_separators = ns; sm->n_segments = nseg; sm->reduced_size = 6 * ns;
    if (!N || !F) { sm->termination = VPGO_TERM_NONE; return VIL_OK; }
    const int nfb = (F + PG_BLK - 1) / PG_BLK, npb = (N + PG_BLK - 1) / PG_BLK, T = P.ld / 16;
    hipStream_t s = c->stream;
    if ((st = put_ctl(c, o)) != VIL_OK) return st;
#define PG_MARK(k, n) VILCHK(c->prof.mark(k, n, s))
    PG_MARK(K_LIN, 1);
    hipLaunchKernelGGL(k_pgo_lin, dim3((F + 63) / 64), dim3(64), 0, s, P, 0);
    PG_MARK(K_REDUCE, 1);
    hipLaunchKernelGGL(k_pgo_reduce, dim3(nfb), dim3(PG_BLK), 0, s, P, 0, nfb);
    PG_MARK(K_DECIDE, 1);
    hipLaunchKernelGGL(k_pgo_decide, dim3(1), dim3(64), 0, s, P, 0, nfb, 0);
    for (int it = 0; it < o->max_iterations; ++it) {
        PG_MARK(K_GATHER, 1);
        hipLaunchKernelGGL(k_pgo_gather, dim3((36 * N + 255) / 256), dim3(256), 0, s, P);
        if (nseg) { PG_MARK(K_SEGMENT, 1); hipLaunchKernelGGL(k_pgo_segment, dim3(nseg), dim3(64), 0, s, P); }
        if (ns) {
            PG_MARK(K_SCHUR, 1);
            hipLaunchKernelGGL(k_pgo_schur, dim3((unsigned)(((size_t)P.ld * P.ld + 255) / 256)), dim3(256), 0, s, P);
            PG_MARK(K_CHOL, T);
            for (int Kt = 0; Kt < T; ++Kt) hipLaunchKernelGGL(k_pgo_chol, dim3(T - Kt), dim3(256), 0, s, P, Kt);
            PG_MARK(K_DBACK, 1);
            hipLaunchKernelGGL(k_pgo_dense_back, dim3(1), dim3(512), 0, s, P);
        }
        PG_MARK(K_SBACK, 1);
        hipLaunchKernelGGL(k_pgo_seg_back, dim3((nseg + ns + 63) / 64), dim3(64), 0, s, P);
        PG_MARK(K_UPDATE, 1);
        hipLaunchKernelGGL(k_pgo_update, dim3((N + 63) / 64), dim3(64), 0, s, P);
        PG_MARK(K_LIN, 1);
        hipLaunchKernelGGL(k_pgo_lin, dim3((F + 63) / 64), dim3(64), 0, s, P, 1);
        PG_MARK(K_REDUCE, 1);
        hipLaunchKernelGGL(k_pgo_reduce, dim3(nfb + npb), dim3(PG_BLK), 0, s, P, 1, nfb);
        PG_MARK(K_DECIDE, 1);
        hipLaunchKernelGGL(k_pgo_decide, dim3(1), dim3(64), 0, s, P, 1, nfb, npb);
    }
    PG_MARK(K_FINISH, 1);
    hipLaunchKernelGGL(k_pgo_finish, dim3((N + 63) / 64), dim3(64), 0, s, P);
    PG_MARK(-1, 0);
#undef PG_MARK
    VILCHK(hipMemcpyAsync(c->h_ctl, P.ctl, sizeof(PgCtl), hipMemcpyDeviceToHost, s));
    VILCHK(hipStreamSynchronize(s));
    VILCHK(hipGetLastError());
    c->prof.collect();
    const PgCtl& k = *c->h_ctl;
    sm->iterations = k.iters; sm->accepted = k.accepted; sm->termination = k.term;
    sm->initial_cost = k.cost0; sm->final_cost = k.cost_cur; sm->final_lambda = k.lambda;
    if (!std::isfinite(k.cost0)) return VIL_ERR_NON_FINITE;
    return VIL_OK;
}

}  // extern "C"
