"""Residual and Jacobian of every factor class of vil_eval_factors / vil_eval_lidar_functors (include/vilsolve.h), restated ONCE from the
reference's definitions over an abstract scalar, plus the instrument that holds an evaluation to it.

  residuals     plain Python over a scalar context S: F64 (Python float = IEEE double) or MP (mpmath, 50 digits).  The module brings its own
                quaternion product, inverse, rotation and slerp (Eigen's conventions); it shares no code with oracle/, tests/numpy_ref.py or
                synth's quaternion helpers.
  Jacobians     forward-mode dual numbers (`Dual`, one partial per evaluation) over that scalar -- nothing is transcribed from the analytic
                Jacobians, except the rows of DEVIATIONS.  Over MP that is the exact derivative of the residual as written, over F64 its
                float64 floor.  Coordinates: local tangent (P += d, Q = Q (x) [1, d/2], derivative at d = 0; the normalisation of
                pose_local_parameterization.cpp:3-18 has derivative 0 there and is left out) for visual, IMU, edge, plane and the four lidar
                functors, column 7 of every pose block exactly 0; the seven raw coordinates [p, qx, qy, qz, qw] for ICP / LPS, which is what
                ceres::Jet<double, 7> holds and what vil_eval_factors returns before tangent_fix.
  IMU           vil_eval_factors returns the WHITENED factor (csrc/vil_eval.hpp, k_eval_imu: U x raw), so the reference is whitened with
                U = chol(cov^-1)^T computed in S from the lower triangle of the record's covariance; the float64 floor carries its conditioning.
                With U in front the raw identity blocks become columns of U: only the zero blocks below U's diagonal stay exact.
  fixture       one carrier window, synth.make_config(2, L=20, n_plane=60, n_edge=40); state and constants overwritten per case (`Case`).
  floors        distance of the F64 dual evaluation from the MP one, maximised per class, case family and block position; at most CAP = 1e-12 in
                every family but those of REPORTED_ONLY (ICP / LPS families keyed by bracket angle and class of t: th = 1e-6, th = 1e-3, in ICP
                th = 1e-2, and t or 1 - t = 1e-9 on the acos branch), where eps / th^2 and eps / t are the reference's own float64 arithmetic:
                each of those is held to 16 x its OWN floor, which is printed.
  violations    what of an evaluation misses `distance <= 16 x max(floor, 2^-52)`, bit-equality where the floor is 0 -- the function the GPU
                test asserts with and tests/test_factors_ref.py shows to reject seeded defects.

Distance of a block: max |x - ref| / max |ref| over the block (over the factor's whole Jacobian where the reference block is all zero); of a residual:
max |x - ref| / max(max |ref|, scale), `scale` being the largest of the terms whose sum or difference the residual is (stated per class below),
so that a residual that is exactly 0 still has a measure.  The MP reference is kept as a (hi, lo) pair of float64 arrays, hi + lo = ref to 106
bits; x - hi is exact in float64 for anything near the reference.

Reference definitions (line numbers of the reference sources, as include/vilsolve.h: vil_factor_class, vil_eval_lidar_functors):
  visual   projection_td_factor.cpp:50-67 (use_td = 0: projection_factor.cpp:21-121, the td terms absent)   scale s max(|x/z|, |pts_j_td|)
  IMU      integration_base.h:175-201, imu_factor.h:60-66; deltaQ utility.h:12-24                           scale |U| x (|tp|+|pt|, 2, |tv|+|vt|, |ba|, |bg|)
  prior    marginalization_factor.cpp:362-383                                                               scale |r0| + |J| |dx|
  ICP      lidar_backend.h:107-169; LPS lidar_backend.h:45-80; Eigen::QuaternionBase::slerp                 scale s max(|PIJ|, |temPIJ|) ; 200
  edge, plane, the four functors   lidarFactor.hpp:12-172 on p_w = Q (RLB^T (p_l - TLB)) + P (window-pose form); PLANE3's unit normal is computed in
           S from j, l, m.  Scales, M the largest coordinate among p_w, a, b: max(|p_w - a| |p_w - b|, M max(|p_w - a|, |p_w - b|)) / |a - b| ;
           max(|n_k p_w,k|, |d|) ; max(|n_k p_w,k|, |n_k j_k|) ; max(|p_w|, |closed|) -- the coordinates the differences are taken of count as terms
  In the two AutoDiff functors t_i = (ti - ta) / (tb - ta), T(tb - ta) and T(ti - ta) are doubles before they become Jets, so both contexts take
  them from float64.  The slerp's branch (|d| >= 1 - eps) and flip (d < 0) come from the dot product in S: exact in MP.

DEVIATIONS lists where the reference's analytic Jacobian is NOT the derivative of its residual; there the reference value is its own formula in S."""
import fractions
import functools
import math
import types

import mpmath
import numpy as np

from mvil_fusion_amd import abi, synth

MARGIN = 16.0                    # a device operation order over a float64 floor (as tests/test_gpu_posegraph.py, tests/preint_ref.py)
EPS = 2.0 ** -52
CAP = 1e-12                      # the project's parity tolerance: no family's floor may exceed it, except those of REPORTED_ONLY
UNBOUNDED = "th=1e-6"
SEEDS = (0, 1)

_mpc = mpmath.mp.clone()
_mpc.dps = 50
F64 = types.SimpleNamespace(name="float64", c=float, sqrt=math.sqrt, sin=math.sin, cos=math.cos, acos=math.acos, zero=0.0, one=1.0, half=0.5)
MP = types.SimpleNamespace(name="mp50", c=_mpc.mpf, sqrt=_mpc.sqrt, sin=_mpc.sin, cos=_mpc.cos, acos=_mpc.acos, zero=_mpc.mpf(0), one=_mpc.mpf(1), half=_mpc.mpf(0.5))
ONE_MINUS_EPS = 1.0 - EPS        # Eigen: Scalar(1) - NumTraits<Scalar>::epsilon()

# Where the reference's analytic Jacobian is not the derivative of its residual.  rows / cols: the 3 x 3 block of the RAW 15 x 30 tangent Jacobian
# (columns pose_i 0..5 | speed-bias_i 6..14 | pose_j 15..20 | speed-bias_j 21..29); order: in theta = Jq_bg dbg; vanishes: the state where it is exact.
# The residual is 2 vec(qt^-1 (x) Qi^-1 (x) Qj) with qt = dq (x) [1, theta / 2] NOT normalised and qt^-1 = conj(qt) / |qt|^2.
DEVIATIONS = (
    dict(name="IMU (R, th_i)", rows=3, cols=3, order=2, vanishes="dbg = 0", line="imu_factor.h:99-100",
         what="-(Qleft(Qj^-1 Qi) Qright(qt)) uses conj(qt) for qt^-1: the formula is |qt|^2 = 1 + |theta|^2 / 4 times the derivative"),
    dict(name="IMU (R, bg_i)", rows=3, cols=12, order=1, vanishes="dbg = 0", line="imu_factor.h:127",
         what="-Qleft(Qj^-1 Qi dq) Jq_bg takes dq for qt and drops d(1 / |qt|^2): off by r_theta theta^T / 2 (first order, times the rotation residual)"),
    dict(name="prior J", rows=None, cols=None, order=0, vanishes="never: by definition", line="marginalization_factor.cpp:384-397",
         what="the Jacobian is the stored matrix, not the derivative of r0 + J dx with its sign flip; held bit for bit, only the residual is differentiated-free"),
)
# (R, th_j), imu_factor.h:153-154, is Qleft(qt^-1 Qi^-1 Qj): the exact derivative at every dbg -- no entry.


# Equivalent float64 formulations of the AutoDiff factors' arithmetic, as bits: 1 a true division in place of ceres' f.a * (1 / g.a); 2 acos' derivative as
# (-1 / sqrt) * v in place of -(v / sqrt); 4 the slerp's dot product summed w first; 8 the numerator f.v - q * g.v of a Jet division as one fused
# multiply-add (what a compiler that contracts makes of it: it keeps sin(0) / sin(th) and 1 - sin(th) / sin(th) from having derivatives that are 0 to
# the bit).  Where terms of size 1 / th^2 cancel, which formulation is lucky on one factor is chance: the float64 floor of ICP / LPS is the largest
# distance over all sixteen (floors()); everything else runs formulation 0.
_VARIANT = 0
VARIANTS = 16


def _fms(a, q, b):
    """a - q * b rounded once (floats), as a fused multiply-add"""
    if _VARIANT & 8 and isinstance(a, float):
        return float(fractions.Fraction(a) - fractions.Fraction(q) * fractions.Fraction(b))
    return a - q * b


# ---- dual numbers ------------------------------------------------------------------------------------------------------------------------
class Dual:
    """a + d e, e^2 = 0; the operand rules of ceres::Jet (jet.h) with one partial"""
    __slots__ = ("a", "d")

    def __init__(self, a, d):
        self.a, self.d = a, d

    def __add__(x, y):
        return Dual(x.a + y.a, x.d + y.d) if isinstance(y, Dual) else Dual(x.a + y, x.d)
    __radd__ = __add__

    def __sub__(x, y):
        return Dual(x.a - y.a, x.d - y.d) if isinstance(y, Dual) else Dual(x.a - y, x.d)

    def __rsub__(x, y):
        return Dual(y - x.a, -x.d)

    def __neg__(x):
        return Dual(-x.a, -x.d)

    def __mul__(x, y):
        return Dual(x.a * y.a, x.a * y.d + x.d * y.a) if isinstance(y, Dual) else Dual(x.a * y, x.d * y)
    __rmul__ = __mul__

    def __truediv__(x, y):
        if isinstance(y, Dual) and _VARIANT & 1:
            q = x.a / y.a
            return Dual(q, _fms(x.d, q, y.d) / y.a)
        if isinstance(y, Dual):                  # jet.h: g_a_inverse = 1 / g.a; f_a_by_g_a = f.a * g_a_inverse; (f.v - f_a_by_g_a * g.v) * g_a_inverse.
            inv = 1 / y.a                        # (with a true division sin(th) / sin(th) would be 1 exactly and hide the eps / th^2 of ceres' own arithmetic)
            q = x.a * inv
            return Dual(q, _fms(x.d, q, y.d) * inv)
        return Dual(x.a / y, x.d / y)

    def __rtruediv__(x, y):
        inv = 1 / x.a
        q = y * inv
        return Dual(q, -(q * x.d) * inv)


def val(x):
    return x.a if isinstance(x, Dual) else x


def der(x, S):
    return x.d if isinstance(x, Dual) else S.zero


def fsqrt(S, x):
    if isinstance(x, Dual):
        r = S.sqrt(x.a)
        return Dual(r, x.d / (r + r))
    return S.sqrt(x)


def fsin(S, x):
    return Dual(S.sin(x.a), S.cos(x.a) * x.d) if isinstance(x, Dual) else S.sin(x)


def facos(S, x, defect=None):
    if isinstance(x, Dual):
        g = (S.one / S.sqrt(S.one - x.a * x.a)) * x.d if _VARIANT & 2 else x.d / S.sqrt(S.one - x.a * x.a)
        return Dual(S.acos(x.a), g if defect == "acos_sign" else -g)
    return S.acos(x)


# ---- vectors and quaternions (w, x, y, z), Eigen's conventions ------------------------------------------------------------------------------
def vadd(a, b):
    return [a[0] + b[0], a[1] + b[1], a[2] + b[2]]


def vsub(a, b):
    return [a[0] - b[0], a[1] - b[1], a[2] - b[2]]


def vscale(s, a):
    return [s * a[0], s * a[1], s * a[2]]


def vdot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def vcross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def matvec(m, v):
    """m: nine scalars, row-major"""
    return [m[0] * v[0] + m[1] * v[1] + m[2] * v[2], m[3] * v[0] + m[4] * v[1] + m[5] * v[2], m[6] * v[0] + m[7] * v[1] + m[8] * v[2]]


def qmul(a, b):
    return (a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
            a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3], a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1])


def qinv(q):
    """Eigen's inverse(): the conjugate over the squared norm"""
    n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]
    return (q[0] / n2, -(q[1] / n2), -(q[2] / n2), -(q[3] / n2))


def qrot(q, v):
    """Eigen's quaternion * vector (_transformVector): v + w (2 u x v) + u x (2 u x v)"""
    u = [q[1], q[2], q[3]]
    uv = vcross(u, v)
    uv = [uv[0] + uv[0], uv[1] + uv[1], uv[2] + uv[2]]
    w = vcross(u, uv)
    return [v[0] + q[0] * uv[0] + w[0], v[1] + q[0] * uv[1] + w[1], v[2] + q[0] * uv[2] + w[2]]


def slerp_dot(a, b):
    if _VARIANT & 4:
        return a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3]
    return a[1] * b[1] + a[2] * b[2] + a[3] * b[3] + a[0] * b[0]


def slerp(S, a, t, b, defect=None):
    """Eigen::QuaternionBase::slerp with Jets: abs(Jet) flips the whole Jet; the branch and the flip read the value"""
    d = slerp_dot(a, b)
    neg = val(d) < 0
    ad = -d if neg else d
    if val(ad) >= S.c(ONE_MINUS_EPS):
        s0, s1 = S.one - t, t
    else:
        th = facos(S, ad, defect)
        st = fsin(S, th)
        s0, s1 = fsin(S, (S.one - t) * th) / st, fsin(S, t * th) / st
    if neg:
        if defect == "flip_s0":
            s0 = -s0
        else:
            s1 = -s1
    return tuple(s0 * a[k] + s1 * b[k] for k in range(4))


def _mag(*xs):
    return max(abs(float(val(x))) for x in xs)


# ---- seeded parameter blocks ----------------------------------------------------------------------------------------------------------------
def pose_tangent(S, p7, k=None):
    """(P, Q) of a pose block [p, qx, qy, qz, qw]; k in 0..5 seeds tangent coordinate k: P[k] += e, or Q (x) [1, e_k / 2]"""
    P = [S.c(p7[0]), S.c(p7[1]), S.c(p7[2])]
    Q = (S.c(p7[6]), S.c(p7[3]), S.c(p7[4]), S.c(p7[5]))
    if k is None:
        return P, Q
    if k < 3:
        P[k] = Dual(P[k], S.one)
    else:
        d = [S.zero, S.zero, S.zero]
        d[k - 3] = Dual(S.zero, S.half)
        Q = qmul(Q, (S.one, d[0], d[1], d[2]))
    return P, Q


def pose_raw(S, p7, k=None):
    """(P, Q) with the raw global coordinate k in 0..6 of [p, qx, qy, qz, qw] seeded"""
    x = [S.c(v) for v in p7]
    if k is not None:
        x[k] = Dual(x[k], S.one)
    return [x[0], x[1], x[2]], (x[6], x[3], x[4], x[5])


def seeded(S, xs, k=None):
    xs = [S.c(v) for v in xs]
    if k is not None:
        xs[k] = Dual(xs[k], S.one)
    return xs


# ---- residuals --------------------------------------------------------------------------------------------------------------------------
def visual_residual(S, c, Pi, Qi, Pj, Qj, tic, qic, lam, td, s, k_tr, use_td, defect=None):
    pts_i, pts_j = [c[0], c[1], c[2]], [c[3], c[4], c[5]]
    if use_td:
        ti, tj = td - c[10] + k_tr * c[12], td - c[11] + k_tr * c[13]
        pts_i = [pts_i[0] - ti * c[6], pts_i[1] - ti * c[7], pts_i[2]]            # velocity.z = 0
        if defect != "visual_no_td_j":
            pts_j = [pts_j[0] - tj * c[8], pts_j[1] - tj * c[9], pts_j[2]]
    pc_i = [pts_i[0] / lam, pts_i[1] / lam, pts_i[2] / lam]
    p_imu_i = vadd(qrot(qic, pc_i), tic)
    p_w = vadd(qrot(Qi, p_imu_i), Pi)
    p_imu_j = qrot(qinv(Qj), vsub(p_w, Pj))
    pc_j = qrot(qinv(qic), vsub(p_imu_j, tic))
    u, v = pc_j[0] / pc_j[2], pc_j[1] / pc_j[2]
    sc = float(val(s)) * _mag(u, v, pts_j[0], pts_j[1])
    return [s * (u - pts_j[0]), s * (v - pts_j[1])], [sc, sc]


def imu_raw_residual(S, c, G, Pi, Qi, sbi, Pj, Qj, sbj):
    """integration_base.h:175-201: the 15 raw residuals, their scales, and the quaternions the analytic blocks are built from"""
    Vi, Bai, Bgi = sbi[0:3], sbi[3:6], sbi[6:9]
    Vj, Baj, Bgj = sbj[0:3], sbj[3:6], sbj[6:9]
    dp, dq, dv, dt = c[0:3], (c[6], c[3], c[4], c[5]), c[7:10], c[16]
    dba, dbg = vsub(Bai, c[10:13]), vsub(Bgi, c[13:16])
    th = matvec(c[35:44], dbg)
    qt = qmul(dq, (S.one, th[0] / 2, th[1] / 2, th[2] / 2))
    vt = vadd(vadd(dv, matvec(c[44:53], dba)), matvec(c[53:62], dbg))
    pt = vadd(vadd(dp, matvec(c[17:26], dba)), matvec(c[26:35], dbg))
    Qi_inv = qinv(Qi)
    tp = qrot(Qi_inv, vsub(vadd(vscale(S.half * dt * dt, G), Pj), vadd(Pi, vscale(dt, Vi))))
    tv = qrot(Qi_inv, vsub(vadd(vscale(dt, G), Vj), Vi))
    qe = qmul(qinv(qt), qmul(Qi_inv, Qj))
    r = vsub(tp, pt) + [2 * qe[1], 2 * qe[2], 2 * qe[3]] + vsub(tv, vt) + vsub(Baj, Bai) + vsub(Bgj, Bgi)
    sc = [_mag(*tp) + _mag(*pt)] * 3 + [2.0] * 3 + [_mag(*tv) + _mag(*vt)] * 3 + [_mag(*Bai, *Baj)] * 3 + [_mag(*Bgi, *Bgj)] * 3
    return r, sc, dict(qt=qt, qe=qe, dq=dq, Qi=Qi, Qj=Qj)


def _ql33(q):
    """bottom-right 3 x 3 of Qleft(q) = w I + [v]x (utility.h:47-54), rows of three"""
    w, x, y, z = q
    return [[w, -z, y], [z, w, -x], [-y, x, w]]


def _qr33(q):
    """bottom-right 3 x 3 of Qright(q) = w I - [v]x (utility.h:57-64)"""
    w, x, y, z = q
    return [[w, z, -y], [-z, w, x], [y, -x, w]]


def _mm(a, b):
    return [[a[i][0] * b[0][j] + a[i][1] * b[1][j] + a[i][2] * b[2][j] for j in range(3)] for i in range(3)]


def imu_analytic_rotation_blocks(S, c, q, defect=None):
    """the reference's formulas for the raw blocks (3, 3) and (3, 12), imu_factor.h:99-100 and :127, from plain scalars"""
    A = qmul(qinv(q["Qj"]), q["Qi"])
    p = q["dq"] if defect == "imu_dq_for_qt" else q["qt"]
    m = _mm(_ql33(A), _qr33(p))                                  # (Qleft Qright) bottom right = -v pv^T + (w I + [v]x)(pw I - [pv]x)
    if defect != "imu_drop_vpv":
        m = [[m[i][j] - A[1 + i] * p[1 + j] for j in range(3)] for i in range(3)]
    b33 = [[-m[i][j] for j in range(3)] for i in range(3)]
    Jq = [c[35:38], c[38:41], c[41:44]]
    m = _mm(_ql33(qmul(A, q["dq"])), Jq)
    b312 = [[-m[i][j] for j in range(3)] for i in range(3)]
    return b33, b312


def sqrt_information(S, cov):
    """U = chol(cov^-1)^T (imu_factor.h:64) from the LOWER triangle of cov (225 scalars): cov = C C^T, W = C^-1, cov^-1 = W^T W = L L^T, U = L^T"""
    def chol(A):
        L = [[S.zero] * 15 for _ in range(15)]
        for j in range(15):
            d = A[j][j]
            for k in range(j):
                d = d - L[j][k] * L[j][k]
            L[j][j] = S.sqrt(d)
            for i in range(j + 1, 15):
                s = A[i][j]
                for k in range(j):
                    s = s - L[i][k] * L[j][k]
                L[i][j] = s / L[j][j]
        return L
    C = chol([[cov[15 * i + j] for j in range(15)] for i in range(15)])
    W = [[S.zero] * 15 for _ in range(15)]
    for j in range(15):
        W[j][j] = S.one / C[j][j]
        for i in range(j + 1, 15):
            s = S.zero
            for k in range(j, i):
                s = s - C[i][k] * W[k][j]
            W[i][j] = s / C[i][i]
    A = [[S.zero] * 15 for _ in range(15)]
    for i in range(15):
        for j in range(i + 1):
            s = S.zero
            for k in range(i, 15):
                s = s + W[k][i] * W[k][j]
            A[i][j] = s
    L = chol(A)
    return [[L[j][i] for j in range(15)] for i in range(15)]


def icp_residual(S, c, pa, pb, pc, pd, defect=None):
    """c: the ten float64 constants; p*: (P, Q)"""
    t_i, t_j = (c[4] - c[0]) / (c[1] - c[0]), (c[5] - c[2]) / (c[3] - c[2])          # doubles in the functor
    wab, tia, wcd, tjc = S.c(c[1] - c[0]), S.c(c[4] - c[0]), S.c(c[3] - c[2]), S.c(c[5] - c[2])
    Qi, Qj = slerp(S, pa[1], S.c(t_i), pb[1], defect), slerp(S, pc[1], S.c(t_j), pd[1], defect)
    Pi = [pa[0][k] + (pb[0][k] - pa[0][k]) / wab * tia for k in range(3)]
    Pj = [pc[0][k] + (pd[0][k] - pc[0][k]) / wcd * tjc for k in range(3)]
    temQ = qmul(qinv(Qj), Qi)
    tem = qrot(qinv(Qi), vsub(Pj, Pi))
    PIJ = [S.c(c[6]), S.c(c[7]), S.c(c[8])]
    RES = qrot(temQ, vsub(PIJ, tem))
    s = S.c(c[9])
    sc = float(c[9]) * (_mag(*PIJ) + _mag(*tem)) * max(1.0, _mag(*temQ)) ** 2
    return [RES[0] * s, S.zero, RES[2] * s], [sc, sc, sc]


def lps_residual(S, c, pa, pb, defect=None):
    t_i = (c[2] - c[0]) / (c[1] - c[0])
    Qi = slerp(S, pa[1], S.c(t_i), pb[1], defect)
    Q12 = qmul(qinv(Qi), (S.c(c[6]), S.c(c[3]), S.c(c[4]), S.c(c[5])))
    two, h = S.c(2.0), S.c(0.01)
    sc = 200.0 * max(1.0, _mag(*Q12))
    return [two * Q12[1] / h, two * Q12[2] / h, two * Q12[3] / h], [sc, sc, sc]


def lidar_world(S, cp, q_lb, t_lb, P, Q):
    """p_w = Q (RLB^T (p_l - TLB)) + P"""
    qlb = (S.c(q_lb[3]), S.c(q_lb[0]), S.c(q_lb[1]), S.c(q_lb[2]))
    pb = qrot(qinv(qlb), vsub(cp, [S.c(t_lb[0]), S.c(t_lb[1]), S.c(t_lb[2])]))
    return vadd(qrot(Q, pb), P)


def lidar_residual(S, kind, c, q_lb, t_lb, P, Q):
    """kind: VIL_LIDAR_EDGE 0, PLANE3 1, PLANE_NORM 2, DISTANCE 3; c: the point's float64 constants"""
    c = [S.c(x) for x in c]
    pw = lidar_world(S, c[0:3], q_lb, t_lb, P, Q)
    if kind == 0:
        a, b = c[3:6], c[6:9]
        da, db = vsub(pw, a), vsub(pw, b)
        nu, de = vcross(da, db), vsub(a, b)
        n = fsqrt(S, vdot(de, de))
        la, lb, m = math.sqrt(float(val(vdot(da, da)))), math.sqrt(float(val(vdot(db, db)))), _mag(*pw, *a, *b)
        sc = max(la * lb, m * max(la, lb)) / float(val(n))
        return [nu[0] / n, nu[1] / n, nu[2] / n], [sc] * 3
    if kind == 1:
        j = c[3:6]
        nv = vcross(vsub(j, c[6:9]), vsub(j, c[9:12]))
        nn = S.sqrt(vdot(nv, nv))
        nv = [nv[0] / nn, nv[1] / nn, nv[2] / nn]
        d = vsub(pw, j)
        return [vdot(d, nv)], [_mag(*[pw[k] * nv[k] for k in range(3)], *[j[k] * nv[k] for k in range(3)])]
    if kind == 2:
        n = c[3:6]
        return [vdot(n, pw) + c[6]], [_mag(n[0] * pw[0], n[1] * pw[1], n[2] * pw[2], c[6])]
    sc = _mag(*pw, *c[3:6])
    return vsub(pw, c[3:6]), [sc] * 3


def prior_residual(S, pr, blocks, defect=None):
    """marginalization_factor.cpp:362-383; blocks: the kept blocks' current values.  Returns (r, scale)."""
    n = pr.n
    dx = [S.zero] * n
    xo = 0
    for b in range(len(pr.blk_kind)):
        gs = 7 if int(pr.blk_kind[b]) in (abi.BLK_POSE, abi.BLK_EX) else (9 if int(pr.blk_kind[b]) == abi.BLK_SPEEDBIAS else 1)
        x, x0, col = [S.c(v) for v in blocks[b]], [S.c(v) for v in pr.x0[xo:xo + gs]], int(pr.blk_col[b])
        xo += gs
        if gs != 7:
            for k in range(gs):
                dx[col + k] = x[k] - x0[k]
            continue
        for k in range(3):
            dx[col + k] = x[k] - x0[k]
        q = qmul(qinv((x0[6], x0[3], x0[4], x0[5])), (x[6], x[3], x[4], x[5]))
        sg = S.c(2.0) if q[0] >= 0 else S.c(-2.0)
        for k in range(3):
            dx[col + 3 + k] = sg * q[1 + k]
        if defect == "prior_flip_translation" and not q[0] >= 0:
            for k in range(3):
                dx[col + k] = -dx[col + k]
    Jm = pr.J_matrix()
    r, sc = [], []
    for i in range(n):
        s, a = S.c(pr.r0[i]), abs(float(pr.r0[i]))
        for k in range(n):
            t = S.c(Jm[i, k]) * dx[k]
            s, a = s + t, a + abs(float(t))
        r.append(s); sc.append(a)
    return r, sc


# ---- cases ------------------------------------------------------------------------------------------------------------------------------------
CLASSES = {"imu": abi.FACTOR_IMU, "visual": abi.FACTOR_VISUAL, "prior": abi.FACTOR_PRIOR, "icp": abi.FACTOR_ICP, "lps": abi.FACTOR_LPS,
           "edge": abi.FACTOR_EDGE, "plane": abi.FACTOR_PLANE}
FUNCTORS = {"f_edge": 0, "f_plane3": 1, "f_plane_norm": 2, "f_distance": 3}
FUNCTOR_NC = {0: 9, 1: 12, 2: 7, 3: 6}
FUNCTOR_NR = {0: 3, 1: 1, 2: 1, 3: 3}
KEYS = tuple(CLASSES) + tuple(FUNCTORS)


class Case:
    """One eval_factors (w) or eval_lidar_functors (consts, q_lb, t_lb, pose) call: key, name, seed and the family of every factor"""

    def __init__(self, key, name, seed, family, w=None, consts=None, q_lb=None, t_lb=None, pose=None, pos_family=None):
        self.key, self.name, self.seed, self.family, self.w = key, name, seed, tuple(family), w
        self.pos_family = pos_family or {}              # block position -> family per factor, where a block has a family of its own (ICP: its bracket's)
        self.consts, self.q_lb, self.t_lb, self.pose = consts, q_lb, t_lb, pose

    @property
    def nfactors(self):
        return len(self.family)

    def fam(self, f, position):
        return self.pos_family[position][f] if position in self.pos_family else self.family[f]

    def label(self, f):
        return "%s/%s seed %d factor %d" % (self.name, self.family[f], self.seed, f)


@functools.lru_cache(maxsize=None)
def carrier():
    return synth.make_config(2, L=20, n_plane=60, n_edge=40)


def copy_window(w):
    w2 = abi.Window(w.K, w.L)
    w2.__dict__.update({k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in w.__dict__.items()})
    return w2


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / math.sqrt(float(v @ v))


def _axis_angle(axis, ang):
    """[x y z w] of the rotation by `ang` about `axis`"""
    a = _unit(axis) * math.sin(ang / 2)
    return np.array([a[0], a[1], a[2], math.cos(ang / 2)])


def _wxyz(q):
    return (float(q[3]), float(q[0]), float(q[1]), float(q[2]))


def _xyzw(q):
    return np.array([q[1], q[2], q[3], q[0]], np.float64)


def _qm(a, b):
    """a (x) b for [x y z w] arrays, normalised"""
    return _unit(_xyzw(qmul(_wxyz(a), _wxyz(b))))


def _qi(a):
    return _xyzw(qinv(_wxyz(a)))


def _rot(q, v):
    return np.array(qrot(_wxyz(q), [float(x) for x in v]))


def _with_sign(q, negative):
    """q or -q so that qw < 0 (negative) or qw > 0"""
    return -q if (q[3] > 0) == negative else q


# visual ---------------------------------------------------------------------------------------------------------------------------------
VIS_FAMILIES = ("generic", "depth 1e-3", "depth 10", "z_j 0.1", "corner 1.5", "td 0.03")
VIS_LANDMARKS = 12


def _visual_window(seed, kind):
    """kind: "td" (families per landmark), "no td" (the same, use_td = 0), "qw<0" (the same, every quaternion negative), "rot 120" (odd
    frames' cameras turned 120 degrees about their y axis; every landmark on the bisector)"""
    rng = np.random.default_rng(100 + seed)
    w = copy_window(carrier())
    K, L = w.K, w.L
    qb = _unit(rng.normal(size=4))
    ex_q = _qm(w.ex_pose[3:], _axis_angle(rng.normal(size=3), 0.05))
    w.ex_pose = np.concatenate([w.ex_pose[:3] + rng.normal(0, 0.005, 3), ex_q])
    small = [_axis_angle(rng.normal(size=3), rng.uniform(0.02, 0.15)) for _ in range(K)]
    turn = _qm(_qm(ex_q, _axis_angle([0, 1, 0], np.deg2rad(120.0))), _qi(ex_q))            # the camera's y axis, in the body frame
    for k in range(K):
        q = _qm(qb, small[k])
        if kind == "rot 120" and k % 2:
            q = _qm(q, turn)
        lateral = rng.normal(0, 1.0, 3) * ([0.15, 0.15, 0.15] if kind == "rot 120" else [3.0, 3.0, 0.02])    # in the base camera's axes: parallax without a change of depth
        w.pose[k] = np.concatenate([_rot(_qm(qb, ex_q), lateral), q])
    w.td = np.array([0.013]); w.tr_over_row = 7e-5; w.use_td = 0 if kind == "no td" else 1
    cam = lambda k, x: _rot(w.pose[k, 3:], _rot(ex_q, x) + w.ex_pose[:3]) + w.pose[k, :3]                 # camera k -> world
    icam = lambda k, X: _rot(_qi(ex_q), _rot(_qi(w.pose[k, 3:]), X - w.pose[k, :3]) - w.ex_pose[:3])      # world -> camera k
    fam_l = [VIS_FAMILIES[l % len(VIS_FAMILIES)] if kind != "rot 120" else "rot 120" for l in range(L)]
    family = [None] * len(w.vis_i)
    for l in range(L):
        fs = np.where(w.vis_l == l)[0]
        i, fam = int(w.vis_i[fs[0]]), fam_l[l]
        uv, depth = rng.uniform(-0.5, 0.5, 2), rng.uniform(2.0, 20.0)
        if fam == "depth 1e-3":
            depth = 1000.0
        elif fam == "depth 10":
            depth = 0.1
        elif fam == "corner 1.5":
            uv = np.array([1.5, -1.45]) * rng.choice([-1.0, 1.0], 2) + rng.normal(0, 0.02, 2)
        if fam == "z_j 0.1":
            X = cam(int(w.vis_j[fs[0]]), 0.1 * np.array([uv[0], uv[1], 1.0]))
        elif fam == "rot 120":
            s60 = math.sin(math.pi / 3) * (1.0 if i % 2 == 0 else -1.0)
            X = cam(i, depth * np.array([s60 + 0.1 * uv[0], 0.2 * uv[1], 0.5]))
        else:
            X = cam(i, depth * np.array([uv[0], uv[1], 1.0]))
        xi = icam(i, X)
        w.inv_depth[l] = 1.0 / xi[2]
        big = fam == "td 0.03"
        vel_i = rng.choice([-5.0, 5.0], 2) * rng.uniform(0.9, 1.1, 2) if big else rng.normal(0, 0.3, 2)
        td_i = w.td[0] - 0.03 if big else w.td[0] - rng.uniform(-0.002, 0.002)
        row_i = rng.uniform(-200, 200)
        for f in fs:
            xj = icam(int(w.vis_j[f]), X)
            vel_j = rng.choice([-5.0, 5.0], 2) * rng.uniform(0.9, 1.1, 2) if big else rng.normal(0, 0.3, 2)
            td_j = w.td[0] - 0.03 if big else w.td[0] - rng.uniform(-0.002, 0.002)
            row_j = rng.uniform(-200, 200)
            c = np.zeros(14)
            c[0:3] = [xi[0] / xi[2], xi[1] / xi[2], 1.0]
            c[3:6] = [xj[0] / xj[2] + rng.normal(0, 1 / 460.0), xj[1] / xj[2] + rng.normal(0, 1 / 460.0), 1.0]
            c[6:8], c[8:10], c[10], c[11], c[12], c[13] = vel_i, vel_j, td_i, td_j, row_i, row_j
            c[0:2] += (w.td[0] - td_i + w.tr_over_row * row_i) * vel_i                           # so that pts_i_td is the projection
            c[3:5] += (w.td[0] - td_j + w.tr_over_row * row_j) * vel_j
            w.vis_const[f] = c
            family[f] = kind if kind in ("no td", "qw<0") else fam
    if kind == "qw<0":
        for k in range(K):
            w.pose[k, 3:] = _with_sign(w.pose[k, 3:], True)
        w.ex_pose[3:] = _with_sign(w.ex_pose[3:], True)
    keep = w.vis_l < VIS_LANDMARKS                    # two landmarks per family: the 50-digit reference costs 20 evaluations per factor
    w.vis_i, w.vis_j, w.vis_l, w.vis_const = w.vis_i[keep], w.vis_j[keep], w.vis_l[keep], w.vis_const[keep]
    return Case("visual", kind, seed, [fam for fam, k in zip(family, keep) if k], w=w)


# IMU ------------------------------------------------------------------------------------------------------------------------------------
def _imu_window(seed, which):
    """which "a": poses with qw > 0, factors 0..8 = dbg 0 | rot 0 | dbg 5e-2 | sum_dt 0.005 | sum_dt 1 | dbg 1e-3 | rot 170 | generic x 2 (rot 0
    makes the whitened (P, bg_i) block cancel the most: it sits on the record whose covariance is conditioned best);
    which "b": poses 0, 3, 6 with qw < 0, the record's dq negative in factors 1, 4, 7"""
    rng = np.random.default_rng(200 + seed)
    w = copy_window(carrier())
    K = w.K
    if seed:
        w.speedbias = w.speedbias + rng.normal(0, 1.0, (K, 9)) * np.array([0.3] * 3 + [0.02] * 3 + [0.002] * 3)
        for k in range(K):
            w.pose[k] = np.concatenate([w.pose[k, :3] + rng.normal(0, 0.05, 3), _qm(w.pose[k, 3:], _axis_angle(rng.normal(size=3), 0.03))])
    neg = (0, 3, 6) if which == "b" else ()
    for k in range(K):
        w.pose[k, 3:] = _with_sign(w.pose[k, 3:], k in neg)
    family = []
    for f in range(K - 1):
        i, j = int(w.imu_i[f]), int(w.imu_j[f])
        c = w.imu_const[f]
        da, dg = _unit(rng.normal(size=3)), _unit(rng.normal(size=3))
        fam, dba, dbg = "generic", 0.02, 1e-4
        if which == "a":
            fam = ("dbg 0", "rot 0", "dbg 5e-2", "sum_dt 0.005", "sum_dt 1", "dbg 1e-3", "rot 170", "generic", "generic")[f]
            if fam in ("dbg 0", "rot 0"):
                dbg = 0.0
            elif fam == "dbg 1e-3":
                dba, dbg = 0.5, 1e-3
            elif fam == "dbg 5e-2":
                dba, dbg = 0.5, 5e-2
            elif fam == "sum_dt 0.005":
                c[16] = 0.005
            elif fam == "sum_dt 1":
                c[16] = 1.0
            if fam in ("rot 0", "rot 170"):
                rel = _qm(_qi(w.pose[i, 3:]), w.pose[j, 3:])
                c[3:7] = rel if fam == "rot 0" else _qm(rel, _axis_angle(rng.normal(size=3), np.deg2rad(170.0)))
            c[3:7] = _with_sign(c[3:7], False)
        else:
            fam = "Qi w<0" if i in neg else ("Qj w<0" if j in neg else "generic")
            c[3:7] = _with_sign(c[3:7], f in (1, 4, 7))
            if f in (1, 4, 7):
                fam = "dq w<0"
        c[10:13] = w.speedbias[i, 3:6] - dba * da
        c[13:16] = w.speedbias[i, 6:9] - dbg * dg if dbg else w.speedbias[i, 6:9]
        family.append(fam)
    return Case("imu", which, seed, family, w=w)


def imu_dbg_is_zero(w, f):
    return bool(np.all(w.speedbias[w.imu_i[f], 6:9] == w.imu_const[f, 13:16]))


# ICP / LPS ------------------------------------------------------------------------------------------------------------------------------------
T_VALUES = (0.0, 0.5, 1.0, 1e-9, 1.0 - 1e-9)
# t = 0, 0.5 and 1 are ONE class: the derivative of sin(t th) / sin(th) is the same difference of two terms of size 1 / th^2 at all three; at the ends
# the two terms are equal to the bit in plain float64, and a compiler that fuses one of the products into the subtraction undoes that (the oracle
# and the device both do).  A family that held t = 0 or 1 alone would have a floor of 0 that no compiled evaluation meets.
T_NAMES = ("t=0|0.5|1", "t=0|0.5|1", "t=0|0.5|1", "t=1e-9", "t=1-1e-9")
BRACKETS = ("th=1e-3", "th=1e-2", "th=1", "th=3", "identical")
ANGLE = {"th=1e-3": 1e-3, "th=1e-2": 1e-2, "th=1": 1.0, "th=3": 3.0}
# A family is (bracket angle, class of t): every bracket meets every t, and a block is bounded by the floor of ITS bracket and ITS class of t.  On the acos branch the
# weights' derivatives are differences of terms of size 1 / th^2 (ceres' Jet division, f.a * (1 / g.a), does not even return 1 for sin(th) / sin(th)),
# and a weight of size t sits next to terms of size 1: the float64 floor of a pose block is about eps / th^2, and about eps / t in the block that t or
# 1 - t = 1e-9 makes small.  That is the reference's own formula in float64; no choice of poses or constants changes it.  The families it puts over
# CAP are listed here per class, each with its reason; they stay in the fixture under the same 16 x bound on their OWN floor, which is printed,
# and tests/test_factors_ref.py asserts that every listed family is over CAP and every other one under it.
_SMALL = "eps / th^2: 1 - x*x in acos' derivative and the difference of the two terms of d(sin(t th) / sin(th))"
_END = "eps / t: the pose block that a weight of 1e-9 makes small is a difference of terms of size 1"
_ENDS = {"%s %s" % (a, t): _END for a in ("th=1e-3", "th=1e-2", "th=1", "th=3") for t in ("t=1e-9", "t=1-1e-9")}
REPORTED_ONLY = {                                        # measured floors, largest block: tests/test_gpu_factors_floor.py
    "lps": {UNBOUNDED: _SMALL, "th=1e-3 t=0|0.5|1": _SMALL, **_ENDS},                                     # th = 1e-2, t = 0.5: 1.1e-13, capped
    "icp": {UNBOUNDED: _SMALL, "th=1e-3 t=0|0.5|1": _SMALL, "th=1e-2 t=0|0.5|1": _SMALL, **_ENDS},       # th = 1e-2, t = 0.5: 2.9e-12 = 1.3 eps / th^2
}
_EXACT_UNIT = ((0.5, 0.5, 0.5, 0.5), (0.5, -0.5, 0.5, -0.5), (0.0, 0.0, 0.0, 1.0), (-0.5, 0.5, 0.5, 0.5))     # q.q = 1 in any order of summation
REL_KINDS = ("plain", "flipped", "tiny")


def reported_only(key, family):
    return family in REPORTED_ONLY.get(key, {})


def _rel_window(seed, kind):
    """Five brackets on the pose pairs (0,1) .. (8,9).  kind "plain": the angles of BRACKETS; "flipped": the same with the second quaternion
    negated; "tiny": th = 1e-6 everywhere, the odd brackets negated.  Five LPS factors, one per bracket; five ICP factors, brackets (k, k + 1) and a
    last one whose four poses are the poses of ONE bracket.  t walks T_VALUES with the bracket, the seed and the kind."""
    rng = np.random.default_rng(300 + seed)
    w = copy_window(carrier())
    off = seed + 2 * (kind == "flipped") + (kind == "tiny")
    labels = []
    for k in range(5):
        lab = UNBOUNDED if kind == "tiny" else BRACKETS[k]
        qa = _unit(rng.normal(size=4))
        if lab == "identical":
            qa = np.array(_EXACT_UNIT[(seed + (kind == "flipped")) % len(_EXACT_UNIT)])
            qb = qa.copy()
        else:
            qb = _qm(qa, _axis_angle(rng.normal(size=3), 2 * ANGLE.get(lab, 1e-6)))      # dot = cos(th): th is HALF the rotation angle
        if kind == "flipped" or (kind == "tiny" and k % 2):
            qb = -qb
        w.pose[2 * k] = np.concatenate([rng.normal(0, 1.0, 3), qa])
        w.pose[2 * k + 1] = np.concatenate([rng.normal(0, 1.0, 3), qb])
        labels.append(lab)                                                      # d < 0 or not: the case's kind and slerp_dots tell
    # bracket k in role p (0 / 1: first / second bracket of an ICP factor, 2: LPS) meets, over the four windows of a kind other than "tiny" (two seeds,
    # plain and flipped), t = 0.5, 1e-9, 1 - 1e-9 and one of the exact ends: every block position of every angle sees every class of t
    tix = lambda k, p: (1, 3, 4, 0 if (k + p) % 2 else 2)[(off + k + p) % 4]
    fam = lambda k, p: labels[k] if kind == "tiny" else labels[k] + " " + T_NAMES[tix(k, p)]      # th = 1e-6: one family whatever t is
    tv = lambda k, p: T_VALUES[tix(k, p)]
    lps_ids, lps_c, lps_fam, icp_ids, icp_c, icp_fam, first, second = [], [], [], [], [], [], [], []
    for k in range(5):
        q = _qm(w.pose[2 * k, 3:], _axis_angle(rng.normal(size=3), 0.1))
        lps_ids.append([2 * k, 2 * k + 1]); lps_c.append([0.0, 0.5, 0.5 * tv(k, 2), q[0], q[1], q[2], q[3]]); lps_fam.append(fam(k, 2))
        a, b = (k, k + 1) if k < 4 else (2, 2)
        icp_ids.append([2 * a, 2 * a + 1, 2 * b, 2 * b + 1])
        icp_c.append([0.0, 0.5, 0.0, 0.5, 0.5 * tv(a, 0), 0.5 * tv(b, 1)] + list(rng.normal(0, 1.0, 3)) + [100.0 / 0.3])
        first.append(fam(a, 0)); second.append(fam(b, 1))
        icp_fam.append(UNBOUNDED if kind == "tiny" else first[-1] + " | " + second[-1])
    w.lps_ids, w.lps_const = np.array(lps_ids, np.int32), np.array(lps_c)
    w.icp_ids, w.icp_const = np.array(icp_ids, np.int32), np.array(icp_c)
    pos = {"pose a": first, "pose b": first, "pose a row 1": first, "pose b row 1": first, "pose c": second, "pose d": second, "pose c row 1": second, "pose d row 1": second}
    return Case("lps", kind, seed, lps_fam, w=w), Case("icp", kind, seed, icp_fam, w=w, pos_family=pos)


def slerp_dots(case):
    """[(factor, bracket, float64 dot, exact dot as (hi, lo))] of every slerp of an ICP / LPS case"""
    w, out = case.w, []
    ids = w.icp_ids if case.key == "icp" else w.lps_ids
    for f in range(len(ids)):
        for s in range(0, ids.shape[1], 2):
            a, b = w.pose[ids[f, s]], w.pose[ids[f, s + 1]]
            d64 = slerp_dot(pose_raw(F64, a)[1], pose_raw(F64, b)[1])
            out.append((f, s // 2, d64, _split(slerp_dot(pose_raw(MP, a)[1], pose_raw(MP, b)[1]))))
    return out


# LiDAR points -------------------------------------------------------------------------------------------------------------------------------
EDGE_FAMILIES = ("generic", "0.3 m", "150 m", "|a-b| 1e-3", "|a-b| 50", "on the line")
PLANE_FAMILIES = ("generic", "0.3 m", "150 m", "on the plane")
PLANE3_FAMILIES = PLANE_FAMILIES + ("sliver",)
DIST_FAMILIES = ("generic", "0.3 m", "150 m", "on the point")


def _lidar_point(rng, fam):
    rad = 0.3 if fam == "0.3 m" else (150.0 if fam == "150 m" else rng.uniform(2.0, 30.0))
    return _unit(rng.normal(size=3)) * rad


def _perp(rng, u):
    v = rng.normal(size=3)
    return _unit(v - (v @ u) * u)


def _lidar_consts(rng, kind, fam, q_lb, t_lb, pose):
    cp = _lidar_point(rng, fam)
    pw = _rot(pose[3:], _rot(_qi(q_lb), cp - t_lb)) + pose[:3]
    if kind == 0:
        u = _unit(rng.normal(size=3))
        half = 5e-4 if fam == "|a-b| 1e-3" else (25.0 if fam == "|a-b| 50" else 0.1)
        off = 0.0 if fam == "on the line" else (0.05 if fam == "|a-b| 1e-3" else rng.uniform(0.02, 0.4))
        c0 = pw + off * _perp(rng, u) + rng.uniform(-0.5, 0.5) * half * u
        return np.concatenate([cp, c0 + half * u, c0 - half * u])
    if kind == 2:
        n = _unit(rng.normal(size=3))
        return np.concatenate([cp, n, [-(n @ pw) + (0.0 if fam == "on the plane" else rng.normal(0, 0.1))]])
    if kind == 1:
        n = _unit(rng.normal(size=3))
        e1 = _perp(rng, n); e2 = np.cross(n, e1)
        j = pw + (0.0 if fam == "on the plane" else rng.normal(0, 0.1)) * n + rng.uniform(0.2, 2.0) * e1 + rng.uniform(0.2, 2.0) * e2
        if fam == "sliver":                                                # j, l, m nearly collinear: the angle at j is 1e-3 rad
            return np.concatenate([cp, j, j + 1.0 * e1, j + 2.0 * e1 + 2e-3 * e2])
        return np.concatenate([cp, j, j + rng.uniform(0.5, 3.0) * e1 + 0.2 * e2, j - 0.3 * e1 + rng.uniform(0.5, 3.0) * e2])
    return np.concatenate([cp, pw + (0.0 if fam == "on the point" else rng.normal(0, 0.2, 3))])


def _lidar_window(seed, negative):
    rng = np.random.default_rng(400 + seed + 10 * negative)
    w = copy_window(carrier())
    w.q_lb, w.t_lb = _unit(rng.normal(size=4)), rng.normal(0, 0.1, 3)
    for k in range(w.K):
        w.pose[k] = np.concatenate([rng.normal(0, 5.0, 3), _with_sign(_unit(rng.normal(size=4)), negative)])
    name = "qw<0" if negative else "qw>0"
    fe = [EDGE_FAMILIES[f % len(EDGE_FAMILIES)] for f in range(len(w.edge_pose))]
    fp = [PLANE_FAMILIES[f % len(PLANE_FAMILIES)] for f in range(len(w.plane_pose))]
    for f, fam in enumerate(fe):
        w.edge_const[f] = _lidar_consts(rng, 0, fam, w.q_lb, w.t_lb, w.pose[w.edge_pose[f]])
    for f, fam in enumerate(fp):
        w.plane_const[f] = _lidar_consts(rng, 2, fam, w.q_lb, w.t_lb, w.pose[w.plane_pose[f]])
    return Case("edge", name, seed, fe, w=w), Case("plane", name, seed, fp, w=w)


def _functor_case(key, seed, negative):
    kind = FUNCTORS[key]
    rng = np.random.default_rng(500 + seed + 10 * negative + 100 * kind)
    q_lb, t_lb = _unit(rng.normal(size=4)), rng.normal(0, 0.1, 3)
    pose = np.concatenate([rng.normal(0, 5.0, 3), _with_sign(_unit(rng.normal(size=4)), negative)])
    fams = (EDGE_FAMILIES, PLANE3_FAMILIES, PLANE_FAMILIES, DIST_FAMILIES)[kind]
    family = [fams[f % len(fams)] for f in range(3 * len(fams))]
    consts = np.array([_lidar_consts(rng, kind, fam, q_lb, t_lb, pose) for fam in family])
    return Case(key, "qw<0" if negative else "qw>0", seed, family, consts=consts, q_lb=q_lb, t_lb=t_lb, pose=pose)


# prior ----------------------------------------------------------------------------------------------------------------------------------
def prior_block_values(w):
    pr = w.prior
    return [{abi.BLK_POSE: lambda i: w.pose[i], abi.BLK_SPEEDBIAS: lambda i: w.speedbias[i], abi.BLK_EX: lambda i: w.ex_pose,
             abi.BLK_TD: lambda i: w.td}[int(k)](int(i)) for k, i in zip(pr.blk_kind, pr.blk_index)]


def _prior_window(seed, flip, size):
    """the state x0 [+] dx with |dx| = size over the prior's n coordinates; flip "none" | "one" | "alternate" | "all": which of the ten pose-type
    blocks (nine poses, the extrinsic) carry the quaternion -q"""
    rng = np.random.default_rng(600 + seed)
    w = copy_window(carrier())
    pr = w.prior
    dx = _unit(rng.normal(size=pr.n)) * size
    xo, nq = 0, 0
    for b in range(len(pr.blk_kind)):
        kind, idx, col = int(pr.blk_kind[b]), int(pr.blk_index[b]), int(pr.blk_col[b])
        if kind in (abi.BLK_POSE, abi.BLK_EX):
            x0 = pr.x0[xo:xo + 7]; xo += 7
            v = dx[col + 3:col + 6] / 2
            q = _qm(x0[3:], np.array([v[0], v[1], v[2], math.sqrt(1.0 - float(v @ v))]))
            if flip == "all" or (flip == "one" and nq == 2) or (flip == "alternate" and nq % 2 == 0):
                q = -q
            nq += 1
            x = np.concatenate([x0[:3] + dx[col:col + 3], q])
            if kind == abi.BLK_POSE:
                w.pose[idx] = x
            else:
                w.ex_pose = x
        elif kind == abi.BLK_SPEEDBIAS:
            w.speedbias[idx] = pr.x0[xo:xo + 9] + dx[col:col + 9]; xo += 9
        else:
            w.td = pr.x0[xo:xo + 1] + dx[col:col + 1]; xo += 1
    return Case("prior", "flip %s" % flip, seed, ["|dx| %g" % size], w=w)


@functools.lru_cache(maxsize=None)
def fixture(key):
    """the cases of one class, both seeds; the windows are shared read-only"""
    out = []
    for seed in SEEDS:
        if key == "visual":
            out += [_visual_window(seed, kind) for kind in ("td", "no td", "qw<0", "rot 120")]
        elif key == "imu":
            out += [_imu_window(seed, which) for which in ("a", "b")]
        elif key in ("icp", "lps"):
            out += [_rel_window(seed, kind)[key == "icp"] for kind in REL_KINDS]
        elif key in ("edge", "plane"):
            out += [_lidar_window(seed, negative)[key == "plane"] for negative in (False, True)]
        elif key == "prior":
            sizes = (1e-9, 0.5) if seed == 0 else (0.5, 1e-9)
            out += [_prior_window(seed, flip, sizes[k // 2]) for k, flip in enumerate(("none", "one", "alternate", "all"))]
        else:
            out += [_functor_case(key, seed, negative) for negative in (False, True)]
    return tuple(out)


def subcase(case, order):
    """The case with only the factors `order`, in that order (the prior has one factor and is returned as it is).  Visual factors must stay grouped by
    landmark in landmark order, so a descending `order` renumbers the landmarks backwards."""
    order = list(order)
    fam = [case.family[f] for f in order]
    if case.w is None:
        return Case(case.key, case.name, case.seed, fam, consts=case.consts[order], q_lb=case.q_lb, t_lb=case.t_lb, pose=case.pose)
    if case.key == "prior":
        return case
    w = copy_window(case.w)
    names = {"imu": ("imu_i", "imu_j", "imu_const"), "visual": ("vis_i", "vis_j", "vis_l", "vis_const"), "icp": ("icp_ids", "icp_const"),
             "lps": ("lps_ids", "lps_const"), "edge": ("edge_pose", "edge_const"), "plane": ("plane_pose", "plane_const")}[case.key]
    for n in names:
        setattr(w, n, getattr(w, n)[order].copy())
    if case.key == "visual" and len(order) > 1 and order[0] > order[-1]:
        w.vis_l = (w.L - 1 - w.vis_l).astype(np.int32)
        w.inv_depth, w.lm_const = w.inv_depth[::-1].copy(), w.lm_const[::-1].copy()
    return Case(case.key, case.name, case.seed, fam, w=w, pos_family={n: [v[f] for f in order] for n, v in case.pos_family.items()})


# ---- evaluation of a case in a scalar context ------------------------------------------------------------------------------------------------
def _visual_eval(S, case, jac, defect):
    w = case.w
    R, SC, J = [], [], []
    s, k_tr = S.c(w.sqrt_info_px), S.c(w.tr_over_row)
    for f in range(len(w.vis_i)):
        c = [S.c(x) for x in w.vis_const[f]]
        i, j, l = int(w.vis_i[f]), int(w.vis_j[f]), int(w.vis_l[f])

        def run(blk, k):
            Pi, Qi = pose_tangent(S, w.pose[i], k if blk == 0 else None)
            Pj, Qj = pose_tangent(S, w.pose[j], k if blk == 1 else None)
            tic, qic = pose_tangent(S, w.ex_pose, k if blk == 2 else None)
            lam = Dual(S.c(w.inv_depth[l]), S.one) if blk == 3 else S.c(w.inv_depth[l])
            td = Dual(S.c(w.td[0]), S.one) if blk == 4 else S.c(w.td[0])
            return visual_residual(S, c, Pi, Qi, Pj, Qj, tic, qic, lam, td, s, k_tr, w.use_td, defect)
        r, sc = run(-1, None)
        R.append(r); SC.append(sc)
        if jac:
            Jf = [S.zero] * 46
            for blk in range(3):
                for k in range(6):
                    d, _ = run(blk, k)
                    Jf[14 * blk + k], Jf[14 * blk + 7 + k] = der(d[0], S), der(d[1], S)
            for blk in (3, 4):
                d, _ = run(blk, 0)
                Jf[42 + 2 * (blk - 3)], Jf[43 + 2 * (blk - 3)] = der(d[0], S), der(d[1], S)
            J.append(Jf)
    return R, SC, J


def imu_raw(S, w, f, jac=True, defect=None):
    """raw residual (15), its scales, the raw 15 x 30 tangent Jacobian by duals (`exact`) and the same with the DEVIATIONS blocks replaced by the
    reference's formulas where dbg != 0 (`reference`)"""
    c = [S.c(x) for x in w.imu_const[f]]
    G = [S.c(x) for x in w.G]
    i, j = int(w.imu_i[f]), int(w.imu_j[f])

    def run(blk, k):
        Pi, Qi = pose_tangent(S, w.pose[i], k if blk == 0 else None)
        Pj, Qj = pose_tangent(S, w.pose[j], k if blk == 2 else None)
        return imu_raw_residual(S, c, G, Pi, Qi, seeded(S, w.speedbias[i], k if blk == 1 else None), Pj, Qj, seeded(S, w.speedbias[j], k if blk == 3 else None))
    r, sc, q = run(-1, None)
    if not jac:
        return r, sc, None, None, q
    exact = [[S.zero] * 30 for _ in range(15)]
    for blk, (c0, n) in enumerate(((0, 6), (6, 9), (15, 6), (21, 9))):
        for k in range(n):
            d = run(blk, k)[0]
            for row in range(15):
                exact[row][c0 + k] = der(d[row], S)
    ref = [row[:] for row in exact]
    if not imu_dbg_is_zero(w, f) or defect in ("imu_dq_for_qt", "imu_drop_vpv"):
        b33, b312 = imu_analytic_rotation_blocks(S, c, q, defect)
        for a in range(3):
            for b in range(3):
                ref[3 + a][3 + b], ref[3 + a][12 + b] = b33[a][b], b312[a][b]
    return r, sc, exact, ref, q


def imu_layout(J30):
    """15 x 30 tangent -> the 480 of Evaluate: [15x7 | 15x9 | 15x7 | 15x9], column 7 of the pose blocks 0"""
    zero = J30[0][0] * 0
    out = []
    for c0, n, pad in ((0, 6, 1), (6, 9, 0), (15, 6, 1), (21, 9, 0)):
        for row in range(15):
            out += list(J30[row][c0:c0 + n]) + [zero] * pad
    return out


def _imu_eval(S, case, jac, defect):
    w = case.w
    R, SC, J = [], [], []
    for f in range(len(w.imu_i)):
        r, sc, _, ref, _ = imu_raw(S, w, f, jac, defect)
        U = sqrt_information(S, [S.c(x) for x in w.imu_const[f, 62:]])
        R.append([sum((U[a][k] * r[k] for k in range(a, 15)), S.zero) for a in range(15)])
        SC.append([sum(abs(float(U[a][k])) * sc[k] for k in range(a, 15)) for a in range(15)])
        if jac:
            J.append(imu_layout([[sum((U[a][k] * ref[k][col] for k in range(a, 15)), S.zero) for col in range(30)] for a in range(15)]))
    return R, SC, J


def _rel_eval(S, case, jac, defect):
    w, icp = case.w, case.key == "icp"
    ids, consts, nb = (w.icp_ids, w.icp_const, 4) if icp else (w.lps_ids, w.lps_const, 2)
    R, SC, J = [], [], []
    for f in range(len(ids)):
        c = [float(x) for x in consts[f]]

        def run(blk, k):
            ps = [pose_raw(S, w.pose[ids[f, b]], k if b == blk else None) for b in range(nb)]
            return icp_residual(S, c, *ps, defect=defect) if icp else lps_residual(S, c, *ps, defect=defect)
        r, sc = run(-1, None)
        R.append(r); SC.append(sc)
        if jac:
            Jf = [S.zero] * (21 * nb)
            for blk in range(nb):
                for k in range(7):
                    d, _ = run(blk, k)
                    for row in range(3):
                        Jf[21 * blk + 7 * row + k] = der(d[row], S)
            J.append(Jf)
    return R, SC, J


def _lidar_eval(S, case, jac, defect):
    if case.w is not None:
        w = case.w
        kind = 0 if case.key == "edge" else 2
        consts, poses = (w.edge_const, w.pose[w.edge_pose]) if kind == 0 else (w.plane_const, w.pose[w.plane_pose])
        q_lb, t_lb = w.q_lb, w.t_lb
    else:
        kind, consts, q_lb, t_lb = FUNCTORS[case.key], case.consts, case.q_lb, case.t_lb
        poses = [case.pose] * len(consts)
    nr = FUNCTOR_NR[kind]
    R, SC, J = [], [], []
    for f in range(len(consts)):
        r, sc = lidar_residual(S, kind, consts[f], q_lb, t_lb, *pose_tangent(S, poses[f]))
        R.append(r); SC.append(sc)
        if jac:
            Jf = [S.zero] * (7 * nr)
            for k in range(6):
                d, _ = lidar_residual(S, kind, consts[f], q_lb, t_lb, *pose_tangent(S, poses[f], k))
                for row in range(nr):
                    Jf[7 * row + k] = der(d[row], S)
            J.append(Jf)
    return R, SC, J


def _prior_eval(S, case, jac, defect):
    w = case.w
    r, sc = prior_residual(S, w.prior, prior_block_values(w), defect)
    J = []
    if jac:                                                 # the stored matrix, by definition (DEVIATIONS)
        Jm = w.prior.J_matrix()
        for b in range(len(w.prior.blk_kind)):
            kind, col = int(w.prior.blk_kind[b]), int(w.prior.blk_col[b])
            gs, ls = {abi.BLK_POSE: (7, 6), abi.BLK_SPEEDBIAS: (9, 9), abi.BLK_EX: (7, 6), abi.BLK_TD: (1, 1)}[kind]
            for i in range(w.prior.n):
                J += [S.c(Jm[i, col + k]) if k < ls else S.zero for k in range(gs)]
    return [r], [sc], [J] if jac else []


def evaluate(S, case, jac=True, defect=None):
    """(R, scale, J): per factor the residuals, their scales (float) and the Jacobian in the layout of vil_eval_factors, as nested lists of S scalars"""
    fn = {"visual": _visual_eval, "imu": _imu_eval, "icp": _rel_eval, "lps": _rel_eval, "prior": _prior_eval}.get(case.key, _lidar_eval)
    return fn(S, case, jac, defect)


def _split(x):
    hi = float(x)
    return hi, float(x - hi)


class Ref:
    """the 50-digit evaluation of a case as float64 pairs: r = r_hi + r_lo, J = J_hi + J_lo; scale per residual"""

    def __init__(self, R, SC, J):
        sp = np.frompyfunc(_split, 1, 2)
        arr = lambda X: [np.asarray(a, np.float64) for a in sp(np.array(X, dtype=object))] if len(X) and len(X[0]) else [np.zeros((len(X), 0))] * 2
        self.r_hi, self.r_lo = arr(R)
        self.J_hi, self.J_lo = arr(J)
        self.scale = np.asarray(SC, np.float64)
        # A block that is 0 by the problem's structure but not by the code's (U's blocks where the covariance has zero blocks) comes out of 50-digit
        # arithmetic as rounding noise, 1e-50 of the factor's terms: it is 0, not a reference value to measure relative distances against.
        for hi, lo in ((self.r_hi, self.r_lo), (self.J_hi, self.J_lo)):
            if hi.size:
                noise = np.abs(hi) < 1e-40 * np.abs(hi).max(axis=1, keepdims=True)
                hi[noise] = 0.0; lo[noise] = 0.0


def as_float(R, J):
    return np.array([[float(x) for x in r] for r in R]), np.array([[float(x) for x in j] for j in J]) if J else np.zeros((len(R), 0))


@functools.lru_cache(maxsize=None)
def reference(key):
    """the 50-digit reference of every case of a class, computed once per process"""
    return tuple(Ref(*evaluate(MP, case)) for case in fixture(key))


@functools.lru_cache(maxsize=None)
def float64_evaluation(key):
    out = []
    for case in fixture(key):
        R, _, J = evaluate(F64, case)
        out.append(as_float(R, J))
    return tuple(out)


# ---- block positions ---------------------------------------------------------------------------------------------------------------------------
IMU_ROWS = ("P", "R", "V", "BA", "BG")
IMU_COLS = ("p_i", "th_i", "v_i", "ba_i", "bg_i", "p_j", "th_j", "v_j", "ba_j", "bg_j")


def imu_index(row, col):
    """index into the 480 of the tangent column col (0..29) of row `row`"""
    for c0, n, base, ld in ((0, 6, 0, 7), (6, 9, 105, 9), (15, 6, 240, 7), (21, 9, 345, 9)):
        if c0 <= col < c0 + n:
            return base + row * ld + col - c0
    raise IndexError(col)


@functools.lru_cache(maxsize=None)
def _positions(key, prior_n=0, prior_nj=0):
    ar = lambda x: np.asarray(x, np.int64)
    if key == "visual":
        rp = [("r", ar([0, 1]))]
        jp = [(n, ar([14 * b + 7 * row + k for row in range(2) for k in range(6)])) for b, n in enumerate(("pose_i", "pose_j", "ex"))]
        jp += [(n + " col 7", ar([14 * b + 6, 14 * b + 13])) for b, n in enumerate(("pose_i", "pose_j", "ex"))]
        jp += [("inv depth", ar([42, 43])), ("td", ar([44, 45]))]
    elif key == "imu":
        rp = [("r " + IMU_ROWS[g], ar([3 * g, 3 * g + 1, 3 * g + 2])) for g in range(5)]
        jp = [("(%s,%s)" % (IMU_ROWS[a], IMU_COLS[b]), ar([imu_index(3 * a + i, 3 * b + j) for i in range(3) for j in range(3)])) for a in range(5) for b in range(10)]
        jp += [("pose_i col 7", ar([7 * row + 6 for row in range(15)])), ("pose_j col 7", ar([240 + 7 * row + 6 for row in range(15)]))]
    elif key in ("icp", "lps"):
        nb = 4 if key == "icp" else 2
        rows = (0, 2) if key == "icp" else (0, 1, 2)
        rp = [("r", ar(rows))] + ([("r row 1", ar([1]))] if key == "icp" else [])
        jp = [("pose %s" % "abcd"[b], ar([21 * b + 7 * row + k for row in rows for k in range(7)])) for b in range(nb)]
        if key == "icp":
            jp += [("pose %s row 1" % "abcd"[b], ar([21 * b + 7 + k for k in range(7)])) for b in range(nb)]
    elif key == "prior":
        rp, jp = [("r", np.arange(prior_n))], [("J", np.arange(prior_nj))]
    else:
        nr = FUNCTOR_NR[{"edge": 0, "plane": 2}.get(key, FUNCTORS.get(key))]
        rp = [("r", np.arange(nr))]
        jp = [("pose", ar([7 * row + k for row in range(nr) for k in range(6)])), ("pose col 7", ar([7 * row + 6 for row in range(nr)]))]
    return tuple(rp), tuple(jp)


def positions(case):
    if case.key == "prior":
        return _positions("prior", case.w.prior.n, case.w.eval_sizes(abi.FACTOR_PRIOR)[1])
    return _positions(case.key)


def distances(case, r, J, ref):
    """{position: (distance per factor, equal-to-the-reference per factor)}; J may be None (residuals only)"""
    rp, jp = positions(case)
    out = {}
    r = np.asarray(r, np.float64).reshape(ref.r_hi.shape)
    err = np.abs((r - ref.r_hi) - ref.r_lo)
    for name, idx in rp:
        den = np.maximum(np.abs(ref.r_hi[:, idx]).max(axis=1), ref.scale[:, idx].max(axis=1))
        out[name] = (err[:, idx].max(axis=1) / np.where(den == 0, 1, den), np.all((r[:, idx] == ref.r_hi[:, idx]) & (ref.r_lo[:, idx] == 0), axis=1))
    if J is not None:
        J = np.asarray(J, np.float64).reshape(ref.J_hi.shape)
        err = np.abs((J - ref.J_hi) - ref.J_lo)
        whole = np.abs(ref.J_hi).max(axis=1)
        for name, idx in jp:
            den = np.abs(ref.J_hi[:, idx]).max(axis=1)
            den = np.where(den == 0, whole, den)                       # a block that is all zero in the reference: against the factor's largest entry
            out[name] = (err[:, idx].max(axis=1) / np.where(den == 0, 1, den), np.all((J[:, idx] == ref.J_hi[:, idx]) & (ref.J_lo[:, idx] == 0), axis=1))
    return out


@functools.lru_cache(maxsize=None)
def floors(key):
    """{(family, position): floor}: the float64 dual evaluation's distance from the 50-digit one, maximised over the fixture's factors of that
    family -- for ICP / LPS over the sixteen formulations of _VARIANT as well.  0 only where float64 reproduces a reference that is itself a float64
    (the structurally exact blocks)."""
    global _VARIANT
    out = {}
    for variant in (range(VARIANTS) if key in ("icp", "lps") else (0,)):
        _VARIANT = variant
        try:
            evals = float64_evaluation(key) if variant == 0 else [as_float(*(lambda R, SC, J: (R, J))(*evaluate(F64, case))) for case in fixture(key)]
        finally:
            _VARIANT = 0
        for case, ref, (r, J) in zip(fixture(key), reference(key), evals):
            for name, (d, eq) in distances(case, r, J, ref).items():
                for f in range(case.nfactors):
                    k = (case.fam(f, name), name)
                    out[k] = max(out.get(k, 0.0), float(d[f]) if not eq[f] else 0.0)
    # UNBOUNDED: terms of size 1 / th^2 = 1e12 cancel, and which pose block an error of 1e-4 lands in -- next to a weight of 1e-9 or of 1 -- is luck
    # per factor and per arithmetic (a fused multiply-add moves it).  Its floor is one number per class: the largest over the pose blocks.
    top = max([v for (fam, n), v in out.items() if fam == UNBOUNDED and n.startswith("pose")], default=0.0)
    for (fam, n), v in out.items():
        if fam == UNBOUNDED and n.startswith("pose") and v > 0:
            out[(fam, n)] = top
    return out


def violations(case, r, J, ref, floor=None, margin=MARGIN):
    """What of one case's evaluation misses `distance <= margin x max(floor, 2^-52)` -- or, where the floor is 0, equality with the reference bit for
    bit -- as a list of (factor label, position, distance, floor).  Empty: the evaluation passes."""
    floor = floor if floor is not None else floors(case.key)
    bad = []
    for name, (d, eq) in distances(case, r, J, ref).items():
        for f in range(case.nfactors):
            fl = floor[(case.fam(f, name), name)]
            if not (eq[f] if fl == 0 else d[f] <= margin * max(fl, EPS)):
                bad.append((case.label(f), name, float(d[f]), fl))
    return bad


def report(key, results, floor=None):
    """results: [(case, distances)].  One line per block position over the capped families -- the largest floor, and the distance, ratio to ITS family's
    floor and place of the worst factor -- and one line per REPORTED_ONLY label.  Returns (lines, worst ratio capped, worst ratio reported only)."""
    floor = floor if floor is not None else floors(key)
    lines, worst, worst_ro, ro = [], 0.0, 0.0, {}
    for name in results[0][1]:
        fl = max([v for (fam, n), v in floor.items() if n == name and not reported_only(key, fam)], default=0.0)
        best, exact = (0.0, 0.0, "-"), True
        for case, ds in results:
            d, eq = ds[name]
            for f in range(case.nfactors):
                fam = case.fam(f, name)
                ff = floor[(fam, name)]
                if ff == 0:
                    exact = exact and bool(eq[f])
                    continue
                ratio = float(d[f]) / max(ff, EPS)
                if reported_only(key, fam):
                    ro[(fam, name)] = max(ro.get((fam, name), (0.0, 0.0, 0.0)), (ratio, float(d[f]), ff))
                elif ratio > best[0]:
                    best = (ratio, float(d[f]), case.label(f))
        if fl == 0 and best[0] == 0.0:
            lines.append("%-12s %-18s bit-equal: %s" % (key, name, "yes" if exact else "NO"))
        else:
            worst = max(worst, best[0])
            lines.append("%-12s %-18s floor %.2e  distance %.2e  ratio %.2f  worst at %s" % (key, name, fl, best[1], best[0], best[2]))
    for (fam, name), (ratio, d, ff) in sorted(ro.items()):
        worst_ro = max(worst_ro, ratio)
        lines.append("%-12s reported only %-20s %-8s floor %.2e  distance %.2e  ratio %.2f" % (key, fam, name, ff, d, ratio))
    return lines, worst, worst_ro


# ---- backends ---------------------------------------------------------------------------------------------------------------------------
def eval_functors(be, kind, consts, q_lb, t_lb, pose, jac=True):
    """vil_eval_lidar_functors / orc_eval_lidar_functors: (r n x nr, J n x nr*7 or None)"""
    import ctypes as C
    n, nr = len(consts), FUNCTOR_NR[kind]
    c = np.ascontiguousarray(consts, dtype=np.float64)
    r, J = np.zeros(n * nr), np.zeros(n * nr * 7)
    dp = C.POINTER(C.c_double)
    f = getattr(be.lib, be.prefix + "eval_lidar_functors"); f.restype = C.c_int
    args = (C.c_int32(kind), C.c_int32(n), c.ctypes.data_as(dp), abi.f64(q_lb).ctypes.data_as(dp), abi.f64(t_lb).ctypes.data_as(dp), abi.f64(pose).ctypes.data_as(dp),
            r.ctypes.data_as(dp), J.ctypes.data_as(dp) if jac else C.cast(None, dp))
    st = f(be.ctx, *args) if be.has_ctx else f(*args)
    assert st == 0, st
    return r.reshape(n, nr), (J.reshape(n, nr * 7) if jac else None)


def backend_eval(be, case, jac=True):
    """(r F x nr, J F x nj or None) of a case through a Backend (the oracle or the device)"""
    if case.w is None:
        return eval_functors(be, FUNCTORS[case.key], case.consts, case.q_lb, case.t_lb, case.pose, jac)
    r, J = be.eval_factors(case.w, CLASSES[case.key], jac=jac)
    F = case.nfactors
    return r.reshape(F, -1).copy(), (J.reshape(F, -1).copy() if jac else None)
