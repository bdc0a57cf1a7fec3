// vilfront_shim.hpp -- header-only C++: the host arithmetic of Estimator::processLidar around vfront_push_scan (vilfront.h), on plain
// arrays.  Three pieces, none of them on the measured path:
//   deskew_motion      estimator.cpp:190-232: the motion TransformToEnd is given, from the two keyframes that bracket the scan;
//   predict_relative   Predict_r, Predict_t, PredictRelative_rt (lidar_frontend.cpp:921-987) and the init_guss of estimator.cpp:285-290;
//   IcpConstraintQueue the first_zv bookkeeping over the LidarICPConstraints deque (:388-411, :423-428, :435) and the six time stamps
//                      (:378-383), on top of classify_icp_constraint (vilicp_shim.hpp).
// Matrices are row-major; quaternions are (w, x, y, z).
//
// A RESTATEMENT WITH A WRITTEN CONTRACT.  Eigen is not available to this project's tests.  The pieces of Eigen 3.3 the reference calls are
// restated below from its text -- Quaternion(Matrix3), slerp, inverse, the product, toRotationMatrix, the fixed-size inverses -- in IEEE
// double (float where the reference casts), one operation per operation written.  They are checked against a 50-digit evaluation of THIS
// text (tests/test_lidarfront_shim.py), NOT against Eigen's bits: Eigen's fixed-size products and inverses may associate differently.
//   quat_from_matrix(m): t = (m00 + m11) + m22.  t > 0: t = sqrt(t + 1), w = 0.5 t, t = 0.5 / t, x = (m21 - m12) t, y = (m02 - m20) t,
//     z = (m10 - m01) t.  Otherwise i = 0; if m11 > m00: i = 1; if m22 > m_ii: i = 2; j = (i + 1) % 3, k = (j + 1) % 3;
//     t = sqrt(((m_ii - m_jj) - m_kk) + 1), q_i = 0.5 t, t = 0.5 / t, w = (m_kj - m_jk) t, q_j = (m_ji + m_ij) t, q_k = (m_ki + m_ik) t.
//   slerp(a, t, b): d = ((a.x b.x + a.y b.y) + a.z b.z) + a.w b.w; absD = |d|; absD >= 1 - epsilon: s0 = 1 - t, s1 = t; otherwise
//     theta = acos(absD), s0 = sin((1 - t) theta) / sin(theta), s1 = sin(t theta) / sin(theta); d < 0: s1 = -s1; s0 a + s1 b per coefficient.
//   inverse(q): n2 = ((x x + y y) + z z) + w w; conjugate / n2 (n2 > 0).
//   a * b: w = ((a.w b.w - a.x b.x) - a.y b.y) - a.z b.z, x = ((a.w b.x + a.x b.w) + a.y b.z) - a.z b.y,
//     y = ((a.w b.y + a.y b.w) + a.z b.x) - a.x b.z, z = ((a.w b.z + a.z b.w) + a.x b.y) - a.y b.x.
//   to_matrix(q): tx = 2 x, ty = 2 y, tz = 2 z, twx = tx w, twy = ty w, twz = tz w, txx = tx x, txy = ty x, txz = tz x, tyy = ty y,
//     tyz = tz y, tzz = tz z; rows (1 - (tyy + tzz), txy - twz, txz + twy), (txy + twz, 1 - (txx + tzz), tyz - twx),
//     (txz - twy, tyz + twx, 1 - (txx + tyy)).
//   3 x 3 and 4 x 4 products: sums over k in ascending order starting from the first product; the 4 x 4 inverse is icp_detail::inv4, the
//     3 x 3 inverse is by cofactors over the determinant (m00 c00 + m01 c01) + m02 c02.
#ifndef VILFRONT_SHIM_HPP
#define VILFRONT_SHIM_HPP

#include <cmath>
#include <deque>
#include <limits>

#include "vilicp_shim.hpp"

namespace vil {
namespace front_detail {

template <class S> struct Quat { S w, x, y, z; };

template <class S>
inline Quat<S> quat_from_matrix(const S* m) {                // m: row-major 3 x 3
    S q[3]; Quat<S> r;
    S t = (m[0] + m[4]) + m[8];
    if (t > S(0)) {
        t = std::sqrt(t + S(1)); r.w = S(0.5) * t; t = S(0.5) / t;
        r.x = (m[7] - m[5]) * t; r.y = (m[2] - m[6]) * t; r.z = (m[3] - m[1]) * t;
        return r;
    }
    int i = 0;
    if (m[4] > m[0]) i = 1;
    if (m[8] > m[4 * i]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    t = std::sqrt(((m[4 * i] - m[4 * j]) - m[4 * k]) + S(1));
    q[i] = S(0.5) * t; t = S(0.5) / t;
    r.w = (m[3 * k + j] - m[3 * j + k]) * t;
    q[j] = (m[3 * j + i] + m[3 * i + j]) * t;
    q[k] = (m[3 * k + i] + m[3 * i + k]) * t;
    r.x = q[0]; r.y = q[1]; r.z = q[2];
    return r;
}

inline Quat<double> slerp(const Quat<double>& a, double t, const Quat<double>& b) {
    const double one = 1.0 - std::numeric_limits<double>::epsilon();
    const double d = ((a.x * b.x + a.y * b.y) + a.z * b.z) + a.w * b.w, absD = std::fabs(d);
    double s0, s1;
    if (absD >= one) { s0 = 1.0 - t; s1 = t; }
    else {
        const double theta = std::acos(absD), sinTheta = std::sin(theta);
        s0 = std::sin((1.0 - t) * theta) / sinTheta;
        s1 = std::sin(t * theta) / sinTheta;
    }
    if (d < 0.0) s1 = -s1;
    return Quat<double>{s0 * a.w + s1 * b.w, s0 * a.x + s1 * b.x, s0 * a.y + s1 * b.y, s0 * a.z + s1 * b.z};
}

inline Quat<double> inverse(const Quat<double>& q) {
    const double n2 = ((q.x * q.x + q.y * q.y) + q.z * q.z) + q.w * q.w;
    if (n2 > 0.0) return Quat<double>{q.w / n2, -q.x / n2, -q.y / n2, -q.z / n2};
    return Quat<double>{0.0, 0.0, 0.0, 0.0};
}

inline Quat<double> mul(const Quat<double>& a, const Quat<double>& b) {
    return Quat<double>{((a.w * b.w - a.x * b.x) - a.y * b.y) - a.z * b.z, ((a.w * b.x + a.x * b.w) + a.y * b.z) - a.z * b.y,
                        ((a.w * b.y + a.y * b.w) + a.z * b.x) - a.x * b.z, ((a.w * b.z + a.z * b.w) + a.x * b.y) - a.y * b.x};
}

inline void to_matrix(const Quat<double>& q, double* R) {
    const double tx = 2.0 * q.x, ty = 2.0 * q.y, tz = 2.0 * q.z;
    const double twx = tx * q.w, twy = ty * q.w, twz = tz * q.w, txx = tx * q.x, txy = ty * q.x, txz = tz * q.x, tyy = ty * q.y, tyz = tz * q.y, tzz = tz * q.z;
    R[0] = 1.0 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
    R[3] = txy + twz; R[4] = 1.0 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1.0 - (txx + tyy);
}

inline void mul3(const double* A, const double* B, double* C) {
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) C[3 * r + c] = (A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c]) + A[3 * r + 2] * B[6 + c];
}
inline void mul3v(const double* A, const double* v, double* o) { for (int r = 0; r < 3; ++r) o[r] = (A[3 * r] * v[0] + A[3 * r + 1] * v[1]) + A[3 * r + 2] * v[2]; }
inline void transpose3(const double* A, double* T) { for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) T[3 * c + r] = A[3 * r + c]; }
inline bool inv3(const double* m, double* o) {
    const double c00 = m[4] * m[8] - m[5] * m[7], c01 = m[5] * m[6] - m[3] * m[8], c02 = m[3] * m[7] - m[4] * m[6];
    const double det = (m[0] * c00 + m[1] * c01) + m[2] * c02;
    if (det == 0.0) return false;
    o[0] = c00 / det; o[1] = (m[2] * m[7] - m[1] * m[8]) / det; o[2] = (m[1] * m[5] - m[2] * m[4]) / det;
    o[3] = c01 / det; o[4] = (m[0] * m[8] - m[2] * m[6]) / det; o[5] = (m[2] * m[3] - m[0] * m[5]) / det;
    o[6] = c02 / det; o[7] = (m[1] * m[6] - m[0] * m[7]) / det; o[8] = (m[0] * m[4] - m[1] * m[3]) / det;
    return true;
}
inline void compose4(const double* R, const double* t, double* M) {
    for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) M[4 * r + c] = R[3 * r + c]; M[4 * r + 3] = t[r]; }
    M[12] = M[13] = M[14] = 0.0; M[15] = 1.0;
}

}  // namespace front_detail

// what current_lidar.vioData holds of the two keyframes that bracket a scan (estimator.cpp:147-164), and the scan's time
struct LidarVio {
    double ti, tj, tl;               // iteri->first + td, iterj->first + td, cloud.time
    double Rwbi[9], Pwbi[3], Vbi[3]; // Rs, Ps, Vs of the left keyframe
    double Rwbj[9], Pwbj[3], Vbj[3]; // of the right one
};

struct DeskewMotion {
    float q[4];                      // transform_es_q (w, x, y, z): vfront_motion.q
    float t[3];                      // transform_es_t: vfront_motion.t
    float time_factor;               // (float)(1 / LidarTimeStep): what vfront_push_scan derives from vfront_options.lidar_time_step
    double tls, tle;                 // the scan's window, tl -+ half a LidarTimeStep
    bool ok;                         // false: trans_lb is singular (the reference would divide by zero)
};

// estimator.cpp:190-232.  RLB, TLB: the LiDAR-body extrinsic.  The two slerps run from temQa to temQb at ss and se; trans_b's rotation is
// (temQle^-1 temQls).toRotationMatrix(), its translation ((-Rwbj^T Pwbj + Rwbj^T Pwbi) LidarTimeStep) / (tj - ti);
// trans_l = (trans_lb trans_b) trans_lb^-1; its rotation block is cast to float and converted to a quaternion IN FLOAT.
inline DeskewMotion deskew_motion(const LidarVio& v, double lidar_time_step, const double* RLB, const double* TLB) {
    using namespace front_detail;
    DeskewMotion m;
    m.time_factor = (float)(1 / lidar_time_step);
    m.tls = v.tl - 0.5 * lidar_time_step; m.tle = v.tl + 0.5 * lidar_time_step;
    const Quat<double> qa = quat_from_matrix<double>(v.Rwbi), qb = quat_from_matrix<double>(v.Rwbj);
    const double ss = (m.tls - v.ti) / (v.tj - v.ti), se = (m.tle - v.ti) / (v.tj - v.ti);
    const Quat<double> qls = slerp(qa, ss, qb), qle = slerp(qa, se, qb);
    double Rb[9], RjT[9], a[3], b[3], tb[3], trans_b[16], trans_lb[16], inv[16], tmp[16], trans_l[16];
    to_matrix(mul(inverse(qle), qls), Rb);
    transpose3(v.Rwbj, RjT);
    for (double& e : RjT) e = -e;
    mul3v(RjT, v.Pwbj, a);                                  // -Rwbj^T Pwbj
    for (double& e : RjT) e = -e;
    mul3v(RjT, v.Pwbi, b);
    for (int k = 0; k < 3; ++k) tb[k] = ((a[k] + b[k]) * lidar_time_step) / (v.tj - v.ti);
    compose4(Rb, tb, trans_b); compose4(RLB, TLB, trans_lb);
    m.ok = icp_detail::inv4(trans_lb, inv);
    if (!m.ok) { for (float& e : m.q) e = 0.f; m.q[0] = 1.f; for (float& e : m.t) e = 0.f; return m; }
    icp_detail::mul4(trans_lb, trans_b, tmp); icp_detail::mul4(tmp, inv, trans_l);
    float Rf[9];
    for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) Rf[3 * r + c] = (float)trans_l[4 * r + c]; m.t[r] = (float)trans_l[4 * r + 3]; }
    const Quat<float> qf = quat_from_matrix<float>(Rf);
    m.q[0] = qf.w; m.q[1] = qf.x; m.q[2] = qf.y; m.q[3] = qf.z;
    return m;
}

// Predict_r (lidar_frontend.cpp:941-964): t = (tl - ti) / (tj - ti); t > 0: slerp(t), otherwise the left keyframe's rotation.  The
// reference calls q.normalized() and DISCARDS the result: the quaternion goes to toRotationMatrix as it is.
inline void predict_r(const LidarVio& v, double* R) {
    using namespace front_detail;
    const Quat<double> qa = quat_from_matrix<double>(v.Rwbi), qb = quat_from_matrix<double>(v.Rwbj);
    const double t = (v.tl - v.ti) / (v.tj - v.ti);
    to_matrix(t > 0 ? slerp(qa, t, qb) : qa, R);
}
// Predict_t (:966-987): dt = tl - ti; dt >= 0: a = (Vbj - Vbi) / (tj - ti), P = (Pwbi + Vbi dt) + ((0.5 a) dt) dt; otherwise Pwbi.
inline void predict_t(const LidarVio& v, double* P) {
    const double dt = v.tl - v.ti;
    for (int k = 0; k < 3; ++k) {
        if (dt >= 0) { const double a = (v.Vbj[k] - v.Vbi[k]) / (v.tj - v.ti); P[k] = (v.Pwbi[k] + v.Vbi[k] * dt) + ((0.5 * a) * dt) * dt; }
        else P[k] = v.Pwbi[k];
    }
}

struct RelativePrediction {
    double Lij[16];                  // TRANSFORM_Lij: the body's motion from scan i to scan j
    double init_guess[16];           // init_guss (estimator.cpp:288-290): the `guess` of vfront_push_scan and of classify_icp_constraint
    double lidar_R_i[9], lidar_T_i[3], lidar_R_j[9], lidar_T_j[3];      // what PredictRelative_rt leaves in both frames' lidarData
    bool ok;                         // false: Rbi is singular
};

// PredictRelative_rt(framei, framej, RLB^T, TBL) (:921-939) and init_guss: R = (RLB tem_r) RLB^T, t = (((RLB tem_r) TBL) + TLB) + RLB tem_t.
// Rbi_bj = Rbi^-1 Rbj with the general 3 x 3 inverse, Tbi_bj = Rbi^T Tbj - Rbi^T Tbi, lidar_R = Rb RBL, lidar_T = Tb + Rb TBL.
inline RelativePrediction predict_relative(const LidarVio& fi, const LidarVio& fj, const double* RLB, const double* TLB, const double* TBL) {
    using namespace front_detail;
    RelativePrediction p;
    double Rbj[9], Rbi[9], Tbj[3], Tbi[3], Rinv[9], RiT[9], Rij[9], a[3], b[3], Tij[3], RBL[9], tmp[3];
    predict_r(fj, Rbj); predict_r(fi, Rbi);
    predict_t(fj, Tbj); predict_t(fi, Tbi);
    transpose3(RLB, RBL);
    p.ok = inv3(Rbi, Rinv);
    if (!p.ok) for (double& e : Rinv) e = 0.0;
    mul3(Rinv, Rbj, Rij);
    transpose3(Rbi, RiT);
    mul3v(RiT, Tbj, a); mul3v(RiT, Tbi, b);
    for (int k = 0; k < 3; ++k) Tij[k] = a[k] - b[k];
    compose4(Rij, Tij, p.Lij);
    mul3(Rbi, RBL, p.lidar_R_i); mul3(Rbj, RBL, p.lidar_R_j);
    mul3v(Rbi, TBL, tmp); for (int k = 0; k < 3; ++k) p.lidar_T_i[k] = Tbi[k] + tmp[k];
    mul3v(Rbj, TBL, tmp); for (int k = 0; k < 3; ++k) p.lidar_T_j[k] = Tbj[k] + tmp[k];
    double RLr[9], Rg[9], tg[3], c[3];
    mul3(RLB, Rij, RLr); mul3(RLr, RBL, Rg);
    mul3v(RLr, TBL, tg); mul3v(RLB, Tij, c);
    for (int k = 0; k < 3; ++k) tg[k] = (tg[k] + TLB[k]) + c[k];
    compose4(Rg, tg, p.init_guess);
    return p;
}

// the image times of a LiDAR frame's two keyframes and its own stamp
struct LidarFrameTimes { double last_image_t, next_image_t, stamp; };

struct QueuedIcpConstraint {
    IcpConstraint c;
    double lidar_ta, lidar_tb, lidar_tc, lidar_td, lidar_ti, lidar_tj;      // :378-383
};

// The LidarICPConstraints deque with first_zv, tem_zv_r and tem_zv_t.  push() is estimator.cpp:378-435 for one classified pair (i, j):
//   cur_R / cur_T are current_lidar's lidar_R / lidar_T: on entry what :294-295 copied from frame j (RelativePrediction.lidar_R_j / _T_j);
//   mode_applied 4, first time (:392-404): tem_zv = cur = frame i's lidar_R / lidar_T, first_zv = false, the deque is popped down to one entry;
//   mode_applied 4, later (:405-410): cur = tem_zv;
//   mode_applied 3 (:423-428): when first_zv is false and the deque holds exactly one entry, that entry is popped and first_zv = true;
//   every pair is pushed (:435), whatever its mode.
class IcpConstraintQueue {
  public:
    std::deque<QueuedIcpConstraint> constraints;
    bool first_zv = true;
    double zv_R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, zv_T[3] = {0, 0, 0};

    void push(const IcpConstraint& c, const LidarFrameTimes& fi, const LidarFrameTimes& fj, const double* lidar_R_i, const double* lidar_T_i, double* cur_R, double* cur_T) {
        QueuedIcpConstraint e;
        e.c = c;
        e.lidar_ta = fi.last_image_t; e.lidar_tb = fi.next_image_t; e.lidar_tc = fj.last_image_t; e.lidar_td = fj.next_image_t; e.lidar_ti = fi.stamp; e.lidar_tj = fj.stamp;
        if (c.mode_applied == 4) {
            if (first_zv) {
                for (int k = 0; k < 9; ++k) zv_R[k] = cur_R[k] = lidar_R_i[k];
                for (int k = 0; k < 3; ++k) zv_T[k] = cur_T[k] = lidar_T_i[k];
                first_zv = false;
                while (constraints.size() > 1) constraints.pop_front();
            } else {
                for (int k = 0; k < 9; ++k) cur_R[k] = zv_R[k];
                for (int k = 0; k < 3; ++k) cur_T[k] = zv_T[k];
            }
        } else if (c.mode_applied == 3) {
            if (!first_zv && constraints.size() == 1) { constraints.pop_front(); first_zv = true; }
        }
        constraints.push_back(e);
    }
};

}  // namespace vil
#endif
