"""include/vilpgo_shim.hpp (ToGtsam / FromGtsam of lidar_mapping, globalMappingIkdTree.cpp:586-598): a small program built with the host compiler
prints matrix and angles for a list of poses; the round trip holds to 1e-15 away from pitch = +-pi/2 and both directions agree with
scipy.spatial.transform.Rotation."""
import os
import subprocess

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r'''
#include <cstdio>
#include "vilpgo_shim.hpp"
int main() {
    vpgo_shim::Pose6D p;
    int fl;
    while (scanf("%lf %lf %lf %lf %lf %lf %d", &p.x, &p.y, &p.z, &p.roll, &p.pitch, &p.yaw, &fl) == 7) {
        double T[16];
        vpgo_shim::to_matrix(p, T, fl != 0);
        const vpgo_shim::Pose6D b = vpgo_shim::from_matrix(T);
        for (int q = 0; q < 16; ++q) printf("%.17g ", T[q]);
        printf("%.17g %.17g %.17g %.17g %.17g %.17g\n", b.x, b.y, b.z, b.roll, b.pitch, b.yaw);
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("pgo_shim")
    src, exe = d / "shim.cpp", d / "shim"
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])

    def run(poses, float_angles=False):
        text = "".join(" ".join(repr(float(v)) for v in p) + " %d\n" % (1 if float_angles else 0) for p in poses)
        out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout
        rows = np.array([[float(v) for v in line.split()] for line in out.splitlines()])
        return rows[:, :16].reshape(-1, 4, 4), rows[:, 16:]
    return run


def poses(n=200, seed=2):
    rng = np.random.default_rng(seed)
    p = np.zeros((n, 6))
    p[:, :3] = 50 * rng.standard_normal((n, 3))
    p[:, 3] = rng.uniform(-np.pi, np.pi, n); p[:, 4] = rng.uniform(-np.pi / 2 + 0.1, np.pi / 2 - 0.1, n); p[:, 5] = rng.uniform(-np.pi, np.pi, n)
    p[0, 3:] = 0.0
    return p


def test_round_trip_and_scipy(shim):
    p = poses()
    T, back = shim(p)
    err = np.abs(back - p)
    err[:, 3:] = np.minimum(err[:, 3:], 2 * np.pi - err[:, 3:])
    print("round trip: largest error %.3e" % err.max())
    assert err.max() <= 1e-15 * max(1.0, np.pi)                         # 1e-15 relative to the angles' range; measured 4.4e-16
    assert np.array_equal(T[:, :3, 3], p[:, :3]) and np.array_equal(T[:, 3], np.tile([0.0, 0.0, 0.0, 1.0], (len(p), 1)))
    want = Rotation.from_euler("ZYX", p[:, [5, 4, 3]]).as_matrix()       # intrinsic z-y'-x'': Rz(yaw) Ry(pitch) Rx(roll)
    assert np.abs(T[:, :3, :3] - want).max() <= 1e-15                    # an entry is three products and a sum on either side: a few roundings of 1.1e-16 each
    ang = Rotation.from_matrix(T[:, :3, :3]).as_euler("ZYX")[:, ::-1]
    d = np.abs(ang - back[:, 3:]); d = np.minimum(d, 2 * np.pi - d)
    assert d.max() <= 1e-14                                              # scipy goes through a quaternion


def test_float_angles_option_rounds_as_the_reference(shim):
    p = poses(20, seed=3)
    T, _ = shim(p, float_angles=True)
    q = p.copy(); q[:, 3:] = q[:, 3:].astype(np.float32).astype(np.float64)
    T2, _ = shim(q)
    assert np.array_equal(T, T2) and not np.array_equal(T, shim(p)[0])


def test_singular_pitch_still_round_trips_the_matrix(shim):
    p = np.array([[1.0, 2.0, 3.0, 0.3, np.pi / 2, -0.7], [0.0, 0.0, 0.0, -1.0, -np.pi / 2, 2.0]])
    T, back = shim(p)
    T2, _ = shim(back)
    assert np.abs(T - T2).max() <= 1e-15
