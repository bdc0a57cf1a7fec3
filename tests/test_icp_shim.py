"""include/vilicp_shim.hpp: classify_icp_constraint against a Python transcription of the rules of Estimator::processLidar
(estimator.cpp:322-421, stateless part) on a table of cases: every mode, the boundaries of every comparison, the ADD_LIDAR_ICP override
and mode 3's information.  Host compiler only, no GPU.  Numbers cross the process boundary as hexadecimal floats, so nothing is rounded."""
import math
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROG = r'''
#include <cstdio>
#include <initializer_list>
#include "vilicp_shim.hpp"
int main() {
    int n = 0;
    if (std::scanf("%d", &n) != 1) return 1;
    for (int k = 0; k < n; ++k) {
        double f, g[16], T[16], E[16]; int add = 0;
        if (std::scanf("%la", &f) != 1) return 1;
        for (double* m : {g, T, E}) for (int i = 0; i < 16; ++i) if (std::scanf("%la", m + i) != 1) return 1;
        if (std::scanf("%d", &add) != 1) return 1;
        const vil::IcpConstraint c = vil::classify_icp_constraint(f, g, T, E, add != 0);
        std::printf("%d %d", c.mode, c.mode_applied);
        for (int i = 0; i < 16; ++i) std::printf(" %a", c.lidar_trans[i]);
        for (int i = 0; i < 6; ++i) std::printf(" %a", c.sqrt_info_diag[i]);
        std::printf("\n");
    }
    return 0;
}
'''


def rot_z(deg):
    a = math.radians(deg)
    return np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1.0]])


def iso(R=None, t=(0, 0, 0)):
    M = np.eye(4)
    if R is not None:
        M[:3, :3] = R
    M[:3, 3] = t
    return M


def transcription(fitness, guess, T, ex_lb, add):
    """:326-421 line by line.  Returns (mode, applied mode, lidar_trans, diagonal of lidar_sqrt_info); unset fields are zeros."""
    tem = guess[:3, 3] - T[:3, 3]
    tem_T = abs(tem[0]) + abs(tem[1]) + abs(tem[2])
    mode = 0
    yaw = math.atan2(guess[1, 0], guess[0, 0]) / math.pi * 180.0                  # Utility::R2ypr(..).x()
    if fitness < 1.0 and tem_T > 0.1:
        mode = 3
    elif fitness < 1.0 and tem_T <= 0.1:
        mode = 2
    elif fitness > 1.0:
        mode = 1
    if abs(T[0, 3]) + abs(T[1, 3]) + abs(T[2, 3]) < 0.01:
        mode = 4 if abs(yaw) < 0.5 else 5
    recorded = mode
    if not add:
        mode = 0
    trans, info = np.zeros((4, 4)), np.zeros(6)
    if mode == 4:
        trans = np.eye(4); info[:] = 1e12
    elif mode == 3:
        trans = np.linalg.inv(ex_lb) @ T @ ex_lb
        info[:] = 1 / fitness * 100
        info[3:] = 500
    return recorded, mode, trans, info


def cases():
    ex = iso(rot_z(90.0) @ np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0.0]]), (0.05, -0.02, 0.1))
    far = iso(rot_z(2.0), (0.0, 0.5, 0.0))                                      # |Tij|_1 = 0.5: not the zero-velocity branch
    up, down = np.nextafter(0.1, 1.0), np.nextafter(0.1, 0.0)
    out = []
    add = lambda name, f, g, T, a=1: out.append((name, float(f), g, T, ex, a))
    add("mode 3", 0.066, iso(rot_z(1.8), (0.4, 0.5, 0.0)), far)
    add("mode 3, fitness 0.0656", 0.0656, iso(rot_z(1.8), (0.2, 0.7, -0.1)), far)
    add("mode 2", 0.3, iso(rot_z(1.8), (0.01, 0.52, 0.0)), far)
    add("mode 1", 1.7, iso(rot_z(1.8), (0.4, 0.5, 0.0)), far)
    add("mode 0: fitness exactly 1", 1.0, iso(rot_z(1.8), (0.4, 0.5, 0.0)), far)
    add("mode 0: fitness exactly 1, small difference", 1.0, iso(rot_z(1.8), (0.0, 0.5, 0.0)), far)
    add("fitness just below 1", np.nextafter(1.0, 0.0), iso(None, (0.4, 0.5, 0.0)), far)
    add("fitness just above 1", np.nextafter(1.0, 2.0), iso(None, (0.4, 0.5, 0.0)), far)
    add("tem_T == 0.1: mode 2", 0.2, iso(None, (0.1, 0.5, 0.0)), far)
    add("tem_T just above 0.1: mode 3", 0.2, iso(None, (up, 0.5, 0.0)), far)
    add("tem_T just below 0.1: mode 2", 0.2, iso(None, (down, 0.5, 0.0)), far)
    still = iso(rot_z(0.01), (0.002, -0.003, 0.001))
    add("mode 4: yaw 0.49", 0.05, iso(rot_z(0.49), (0.3, 0, 0)), still)
    add("mode 5: yaw 0.51", 0.05, iso(rot_z(0.51), (0.3, 0, 0)), still)
    add("mode 4: yaw -0.49", 2.0, iso(rot_z(-0.49), (0.0, 0, 0)), still)
    add("mode 5: yaw -0.51", 2.0, iso(rot_z(-0.51), (0.0, 0, 0)), still)
    add("|Tij|_1 just below 0.01", 0.05, iso(None, (0.3, 0, 0)), iso(None, (np.nextafter(0.01, 0.0), 0, 0)))
    add("|Tij|_1 == 0.01: not zero velocity", 0.05, iso(None, (0.3, 0, 0)), iso(None, (0.01, 0, 0)))
    add("ADD_LIDAR_ICP off, mode 3", 0.066, iso(rot_z(1.8), (0.4, 0.5, 0.0)), far, 0)
    add("ADD_LIDAR_ICP off, mode 4", 0.05, iso(rot_z(0.1), (0.3, 0, 0)), still, 0)
    return out


def run_shim(table):
    lines = [str(len(table))]
    for _, f, g, T, ex, a in table:
        lines.append(" ".join([f.hex()] + [float(v).hex() for m in (g, T, ex) for v in m.reshape(16)] + [str(a)]))
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.cpp"), os.path.join(d, "t")
        open(src, "w").write(PROG)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = subprocess.check_output([exe], input="\n".join(lines) + "\n", text=True).strip().split("\n")
    res = []
    for l in out:
        w = l.split()
        res.append((int(w[0]), int(w[1]), np.array([float.fromhex(v) for v in w[2:18]]).reshape(4, 4), np.array([float.fromhex(v) for v in w[18:24]])))
    return res


def test_classify_matches_the_transcription_on_every_case():
    table = cases()
    got = run_shim(table)
    assert len(got) == len(table)
    modes = {}
    for (name, f, g, T, ex, a), (mode, applied, trans, info) in zip(table, got):
        e_mode, e_applied, e_trans, e_info = transcription(f, g, T, ex, a)
        assert (mode, applied) == (e_mode, e_applied), name
        assert np.array_equal(info, e_info), (name, info, e_info)                # the same double operations in the same order
        # lidar_trans: two 4 x 4 products and one inverse of matrices with entries of order 1 and condition number near 1: some tens of
        # roundings of 1.1e-16 each on either side; 1e-12 is two orders above that and six below the centimetre the factor resolves
        assert np.abs(trans - e_trans).max() <= 1e-12, name
        modes[name] = (mode, applied)
    assert sorted({m for m, _ in modes.values()}) == [0, 1, 2, 3, 4, 5]
    assert modes["mode 0: fitness exactly 1"] == (0, 0) and modes["mode 0: fitness exactly 1, small difference"] == (0, 0)
    assert modes["fitness just below 1"] == (3, 3) and modes["fitness just above 1"] == (1, 1)
    assert modes["tem_T == 0.1: mode 2"] == (2, 2) and modes["tem_T just above 0.1: mode 3"] == (3, 3) and modes["tem_T just below 0.1: mode 2"] == (2, 2)
    assert modes["mode 4: yaw 0.49"] == (4, 4) and modes["mode 5: yaw 0.51"] == (5, 5) and modes["mode 4: yaw -0.49"] == (4, 4) and modes["mode 5: yaw -0.51"] == (5, 5)
    assert modes["|Tij|_1 just below 0.01"] == (4, 4) and modes["|Tij|_1 == 0.01: not zero velocity"] == (3, 3)
    assert modes["ADD_LIDAR_ICP off, mode 3"] == (3, 0) and modes["ADD_LIDAR_ICP off, mode 4"] == (4, 0)


def test_mode_3_information_and_transform():
    table = cases()
    (mode, applied, trans, info), = run_shim(table[:1])
    name, f, g, T, ex, _ = table[0]
    assert (mode, applied, f) == (3, 3, 0.066)
    assert info.tolist() == [1 / 0.066 * 100] * 3 + [500.0] * 3
    assert abs(info[0] - 1515.1515151515152) < 1e-9
    assert np.abs(ex @ trans - T @ ex).max() <= 1e-12                            # EX_LB lidar_trans = T EX_LB
    (_, _, t4, i4), = run_shim([r for r in table if r[0] == "mode 4: yaw 0.49"])
    assert np.array_equal(t4, np.eye(4)) and i4.tolist() == [1e12] * 6
    (_, _, t0, i0), = run_shim([r for r in table if r[0] == "mode 2"])
    assert not t0.any() and not i0.any()
