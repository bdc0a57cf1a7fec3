// vilpgo_shim.hpp -- the two conversions lidar_mapping does at the boundary of its pose graph (globalMappingIkdTree.cpp:586-598), for a caller
// that replaces the GTSAM back end by include/vilpgo.h.  Header-only host C++, no HIP.
//
//   ToGtsam    Pose6D -> Pose3:  Rot3::RzRyRx(x, y, z) of the Euler angles of the reference's own Quaternion (include/global_mapping/Quaternion.h),
//              R = Rz(yaw) Ry(pitch) Rx(roll), and the translation                                  -> vpgo_shim::to_matrix
//   FromGtsam  Pose3 -> Pose6D:  roll, pitch, yaw of the rotation and the translation               -> vpgo_shim::from_matrix
//
// Angles: roll = atan2(R21, R22), pitch = atan2(-R20, sqrt(R21^2 + R22^2)), yaw = atan2(R10, R00) -- the formulas of Quaternion::toEuler and of
// Rot3::roll / pitch / yaw away from pitch = +-pi/2; at the singularity roll and yaw are not separately defined and the pair returned is one of
// the solutions (the matrix still round-trips).
// DEVIATION: Quaternion::toEuler rounds its three angles to float before ToGtsam uses them.  to_matrix works in double; float_angles = true
// applies that rounding for a caller that wants the reference's numbers.
#pragma once
#include <cmath>

namespace vpgo_shim {

struct Pose6D { double x, y, z, roll, pitch, yaw; };      // the layout of aloam_velodyne/common.h

// row-major 4 x 4, as vpgo_add_pose takes it
inline void to_matrix(const Pose6D& p, double* T16, bool float_angles = false) {
    const double r = float_angles ? (double)(float)p.roll : p.roll, q = float_angles ? (double)(float)p.pitch : p.pitch, y = float_angles ? (double)(float)p.yaw : p.yaw;
    const double sr = std::sin(r), cr = std::cos(r), sp = std::sin(q), cp = std::cos(q), sy = std::sin(y), cy = std::cos(y);
    T16[0] = cy * cp; T16[1] = cy * sp * sr - sy * cr; T16[2] = cy * sp * cr + sy * sr; T16[3] = p.x;
    T16[4] = sy * cp; T16[5] = sy * sp * sr + cy * cr; T16[6] = sy * sp * cr - cy * sr; T16[7] = p.y;
    T16[8] = -sp;     T16[9] = cp * sr;                T16[10] = cp * cr;               T16[11] = p.z;
    T16[12] = 0.0; T16[13] = 0.0; T16[14] = 0.0; T16[15] = 1.0;
}

inline Pose6D from_matrix(const double* T16) {
    Pose6D p;
    p.x = T16[3]; p.y = T16[7]; p.z = T16[11];
    p.roll = std::atan2(T16[9], T16[10]);
    p.pitch = std::atan2(-T16[8], std::sqrt(T16[9] * T16[9] + T16[10] * T16[10]));
    p.yaw = std::atan2(T16[4], T16[0]);
    return p;
}

}  // namespace vpgo_shim
