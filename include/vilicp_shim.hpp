// vilicp_shim.hpp -- header-only C++: what Estimator::processLidar does with the fitness score of its scan-to-scan alignment
// (estimator.cpp:322-421), on plain arrays: the constraint mode and, for the two modes optimization() consumes (:1354, :1376), the
// relative transform and the square-root information of the ICP factor.  The score itself is vloop_score (villoop.h) at the
// alignment's result.  Stateless part only: the first_zv bookkeeping over the LidarICPConstraints deque (:392-410, :423-428) and the
// time stamps (:378-383) are IcpConstraintQueue of vilfront_shim.hpp.  Host logic only; nothing here is on the measured path.
#ifndef VILICP_SHIM_HPP
#define VILICP_SHIM_HPP

#include <cmath>

namespace vil {

struct IcpConstraint {
    int mode;                    // constraint_mode as current_lidar.lidarData.mode records it (:372), before the ADD_LIDAR_ICP override
    int mode_applied;            // after the override (:373-376): what LidarICPConstraint.constraint_mode carries into the window
    double lidar_trans[16];      // row-major 4x4; set for mode_applied 3 and 4, zeros otherwise (the reference leaves it unset)
    double sqrt_info_diag[6];    // the diagonal of lidar_sqrt_info ([rotation | translation]); the matrix is diagonal; zeros likewise
};

namespace icp_detail {
// yaw of Utility::R2ypr (utility.h:66-81) in degrees; R row-major inside a 4x4
inline double yaw_deg(const double* M) { return std::atan2(M[4], M[0]) / M_PI * 180.0; }
inline void mul4(const double* A, const double* B, double* C) {
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) { double s = 0.0; for (int k = 0; k < 4; ++k) s += A[4 * r + k] * B[4 * k + c]; C[4 * r + c] = s; }
}
// general 4x4 inverse by cofactors, as a fixed-size Matrix4d::inverse(); false for a singular matrix
inline bool inv4(const double* m, double* o) {
    double v[16];
    v[0] = m[5] * m[10] * m[15] - m[5] * m[11] * m[14] - m[9] * m[6] * m[15] + m[9] * m[7] * m[14] + m[13] * m[6] * m[11] - m[13] * m[7] * m[10];
    v[4] = -m[4] * m[10] * m[15] + m[4] * m[11] * m[14] + m[8] * m[6] * m[15] - m[8] * m[7] * m[14] - m[12] * m[6] * m[11] + m[12] * m[7] * m[10];
    v[8] = m[4] * m[9] * m[15] - m[4] * m[11] * m[13] - m[8] * m[5] * m[15] + m[8] * m[7] * m[13] + m[12] * m[5] * m[11] - m[12] * m[7] * m[9];
    v[12] = -m[4] * m[9] * m[14] + m[4] * m[10] * m[13] + m[8] * m[5] * m[14] - m[8] * m[6] * m[13] - m[12] * m[5] * m[10] + m[12] * m[6] * m[9];
    v[1] = -m[1] * m[10] * m[15] + m[1] * m[11] * m[14] + m[9] * m[2] * m[15] - m[9] * m[3] * m[14] - m[13] * m[2] * m[11] + m[13] * m[3] * m[10];
    v[5] = m[0] * m[10] * m[15] - m[0] * m[11] * m[14] - m[8] * m[2] * m[15] + m[8] * m[3] * m[14] + m[12] * m[2] * m[11] - m[12] * m[3] * m[10];
    v[9] = -m[0] * m[9] * m[15] + m[0] * m[11] * m[13] + m[8] * m[1] * m[15] - m[8] * m[3] * m[13] - m[12] * m[1] * m[11] + m[12] * m[3] * m[9];
    v[13] = m[0] * m[9] * m[14] - m[0] * m[10] * m[13] - m[8] * m[1] * m[14] + m[8] * m[2] * m[13] + m[12] * m[1] * m[10] - m[12] * m[2] * m[9];
    v[2] = m[1] * m[6] * m[15] - m[1] * m[7] * m[14] - m[5] * m[2] * m[15] + m[5] * m[3] * m[14] + m[13] * m[2] * m[7] - m[13] * m[3] * m[6];
    v[6] = -m[0] * m[6] * m[15] + m[0] * m[7] * m[14] + m[4] * m[2] * m[15] - m[4] * m[3] * m[14] - m[12] * m[2] * m[7] + m[12] * m[3] * m[6];
    v[10] = m[0] * m[5] * m[15] - m[0] * m[7] * m[13] - m[4] * m[1] * m[15] + m[4] * m[3] * m[13] + m[12] * m[1] * m[7] - m[12] * m[3] * m[5];
    v[14] = -m[0] * m[5] * m[14] + m[0] * m[6] * m[13] + m[4] * m[1] * m[14] - m[4] * m[2] * m[13] - m[12] * m[1] * m[6] + m[12] * m[2] * m[5];
    v[3] = -m[1] * m[6] * m[11] + m[1] * m[7] * m[10] + m[5] * m[2] * m[11] - m[5] * m[3] * m[10] - m[9] * m[2] * m[7] + m[9] * m[3] * m[6];
    v[7] = m[0] * m[6] * m[11] - m[0] * m[7] * m[10] - m[4] * m[2] * m[11] + m[4] * m[3] * m[10] + m[8] * m[2] * m[7] - m[8] * m[3] * m[6];
    v[11] = -m[0] * m[5] * m[11] + m[0] * m[7] * m[9] + m[4] * m[1] * m[11] - m[4] * m[3] * m[9] - m[8] * m[1] * m[7] + m[8] * m[3] * m[5];
    v[15] = m[0] * m[5] * m[10] - m[0] * m[6] * m[9] - m[4] * m[1] * m[10] + m[4] * m[2] * m[9] + m[8] * m[1] * m[6] - m[8] * m[2] * m[5];
    const double det = m[0] * v[0] + m[1] * v[4] + m[2] * v[8] + m[3] * v[12];
    if (det == 0.0) return false;
    for (int i = 0; i < 16; ++i) o[i] = v[i] / det;
    return true;
}
}  // namespace icp_detail

// fitness: getFitnessScore() at T (:303).  init_guess: the Matrix4d init_guss handed to align (:288-290), T: getFinalTransformation()
// cast to double (:313), EX_LB: the LiDAR-body extrinsic, all row-major 4x4.  add_lidar_icp: ADD_LIDAR_ICP.
//   tem_T = |init_guess.t - T.t|_1 (:327-328);  mode 3: fitness < 1.0 and tem_T > 0.1;  mode 2: fitness < 1.0 and tem_T <= 0.1;
//   mode 1: fitness > 1.0;  fitness == 1.0 exactly (or NaN) matches no branch and stays 0 (:340-353);
//   |T.t|_1 < 0.01 overrides all of them: mode 4 when |yaw(init_guess)| < 0.5 degrees (zero velocity), else mode 5 (pure rotation) (:355-371).
//   mode 4: identity, 1e12 on the diagonal (:390-391);  mode 3: EX_LB^-1 T EX_LB, 1 / fitness * 100 on entries 0-2, 500 on 3-5 (:415-421).
// For every other applied mode the reference leaves both fields unset: zeros here.
inline IcpConstraint classify_icp_constraint(double fitness, const double* init_guess, const double* T, const double* EX_LB, bool add_lidar_icp) {
    IcpConstraint c;
    for (int i = 0; i < 16; ++i) c.lidar_trans[i] = 0.0;
    for (int i = 0; i < 6; ++i) c.sqrt_info_diag[i] = 0.0;
    const double tem_T = std::fabs(init_guess[3] - T[3]) + std::fabs(init_guess[7] - T[7]) + std::fabs(init_guess[11] - T[11]);
    int mode = 0;
    if (fitness < 1.0 && tem_T > 0.1) mode = 3;
    else if (fitness < 1.0 && tem_T <= 0.1) mode = 2;
    else if (fitness > 1.0) mode = 1;
    if (std::fabs(T[3]) + std::fabs(T[7]) + std::fabs(T[11]) < 0.01) mode = std::fabs(icp_detail::yaw_deg(init_guess)) < 0.5 ? 4 : 5;
    c.mode = mode;
    c.mode_applied = add_lidar_icp ? mode : 0;
    if (c.mode_applied == 4) {
        for (int i = 0; i < 4; ++i) c.lidar_trans[5 * i] = 1.0;
        for (int i = 0; i < 6; ++i) c.sqrt_info_diag[i] = 1e12;
    } else if (c.mode_applied == 3) {
        double inv[16], tmp[16];
        if (icp_detail::inv4(EX_LB, inv)) { icp_detail::mul4(inv, T, tmp); icp_detail::mul4(tmp, EX_LB, c.lidar_trans); }
        for (int i = 0; i < 3; ++i) { c.sqrt_info_diag[i] = 1 / fitness * 100; c.sqrt_info_diag[3 + i] = 500.0; }
    }
    return c;
}

}  // namespace vil
#endif
