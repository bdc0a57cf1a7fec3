"""include/vilfront_shim.hpp: deskew_motion, predict_relative and IcpConstraintQueue compiled into a small program (g++ only, no GPU) and
checked against a Python restatement written from the reference lines the header names: mpmath at 50 digits for the quaternion paths,
plain Python for the deque."""
import os
import subprocess

import mpmath
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROG = r'''
#include <cstdio>
#include <cstring>
#include "vilfront_shim.hpp"
static bool rd(double* v, int n) { for (int i = 0; i < n; ++i) if (std::scanf("%la", v + i) != 1) return false; return true; }
static void pr(const double* v, int n) { for (int i = 0; i < n; ++i) std::printf(" %a", v[i]); }
static bool rdvio(vil::LidarVio& v) { return rd(&v.ti, 1) && rd(&v.tj, 1) && rd(&v.tl, 1) && rd(v.Rwbi, 9) && rd(v.Pwbi, 3) && rd(v.Vbi, 3) && rd(v.Rwbj, 9) && rd(v.Pwbj, 3) && rd(v.Vbj, 3); }
int main() {
    char cmd[8];
    vil::IcpConstraintQueue Q;
    while (std::scanf("%7s", cmd) == 1) {
        if (cmd[0] == 'M') {
            vil::LidarVio v; double step, RLB[9], TLB[3];
            if (!rdvio(v) || !rd(&step, 1) || !rd(RLB, 9) || !rd(TLB, 3)) return 1;
            const vil::DeskewMotion m = vil::deskew_motion(v, step, RLB, TLB);
            std::printf("M %d", (int)m.ok);
            for (float f : m.q) std::printf(" %a", (double)f);
            for (float f : m.t) std::printf(" %a", (double)f);
            std::printf(" %a %a %a\n", (double)m.time_factor, m.tls, m.tle);
        } else if (cmd[0] == 'P') {
            vil::LidarVio a, b; double RLB[9], TLB[3], TBL[3];
            if (!rdvio(a) || !rdvio(b) || !rd(RLB, 9) || !rd(TLB, 3) || !rd(TBL, 3)) return 1;
            const vil::RelativePrediction p = vil::predict_relative(a, b, RLB, TLB, TBL);
            std::printf("P %d", (int)p.ok);
            pr(p.Lij, 16); pr(p.init_guess, 16); pr(p.lidar_R_i, 9); pr(p.lidar_T_i, 3); pr(p.lidar_R_j, 9); pr(p.lidar_T_j, 3);
            std::printf("\n");
        } else if (cmd[0] == 'Q') {
            double mode[2], ti[3], tj[3], Ri[9], Ti[3], Rc[9], Tc[3];
            if (!rd(mode, 2) || !rd(ti, 3) || !rd(tj, 3) || !rd(Ri, 9) || !rd(Ti, 3) || !rd(Rc, 9) || !rd(Tc, 3)) return 1;
            vil::IcpConstraint c; std::memset(&c, 0, sizeof c); c.mode = (int)mode[0]; c.mode_applied = (int)mode[1];
            Q.push(c, vil::LidarFrameTimes{ti[0], ti[1], ti[2]}, vil::LidarFrameTimes{tj[0], tj[1], tj[2]}, Ri, Ti, Rc, Tc);
            std::printf("Q %a %a", (double)Q.constraints.size(), (double)Q.first_zv);
            pr(Rc, 9); pr(Tc, 3);
            for (const vil::QueuedIcpConstraint& e : Q.constraints) { const double s[8] = {(double)e.c.mode, (double)e.c.mode_applied, e.lidar_ta, e.lidar_tb, e.lidar_tc, e.lidar_td, e.lidar_ti, e.lidar_tj}; pr(s, 8); }
            std::printf("\n");
        } else return 2;
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("frontshim")
    (d / "p.cpp").write_text(PROG)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "include"), str(d / "p.cpp"), "-o", str(d / "p")])
    return str(d / "p")


def run(exe, lines):
    text = "\n".join(l[0] + " " + " ".join(float(v).hex() for v in l[1]) for l in lines)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout
    return [(l.split()[0], [float.fromhex(v) for v in l.split()[1:]]) for l in out.splitlines()]


# ---- the restatement at 50 digits, from estimator.cpp:190-232 and lidar_frontend.cpp:921-987 --------------------------------------------
mpf = mpmath.mpf


@pytest.fixture(autouse=True)
def _fifty_digits():
    with mpmath.workdps(50):
        yield


EPS64 = float(np.finfo(np.float64).eps)


def M(a, r, c):
    return mpmath.matrix([[mpf(float(a[i * c + j])) for j in range(c)] for i in range(r)])


def quat_of(R):
    """Quaternion(Matrix3) of Eigen, (w, x, y, z): the branch by the trace, then by the largest diagonal entry"""
    t = R[0, 0] + R[1, 1] + R[2, 2]
    if t > 0:
        t = mpmath.sqrt(t + 1)
        return [t / 2, (R[2, 1] - R[1, 2]) / (2 * t), (R[0, 2] - R[2, 0]) / (2 * t), (R[1, 0] - R[0, 1]) / (2 * t)]
    i = 0
    if R[1, 1] > R[0, 0]: i = 1
    if R[2, 2] > R[i, i]: i = 2
    j, k = (i + 1) % 3, (i + 2) % 3
    t = mpmath.sqrt(R[i, i] - R[j, j] - R[k, k] + 1)
    q = [None] * 4
    q[1 + i] = t / 2; q[0] = (R[k, j] - R[j, k]) / (2 * t); q[1 + j] = (R[j, i] + R[i, j]) / (2 * t); q[1 + k] = (R[k, i] + R[i, k]) / (2 * t)
    return q


def slerp(a, t, b):
    d = sum(x * y for x, y in zip(a, b))
    if abs(d) >= 1 - mpf(EPS64):
        s0, s1 = 1 - t, t
    else:
        th = mpmath.acos(abs(d)); s0, s1 = mpmath.sin((1 - t) * th) / mpmath.sin(th), mpmath.sin(t * th) / mpmath.sin(th)
    if d < 0:
        s1 = -s1
    return [s0 * x + s1 * y for x, y in zip(a, b)]


def qmul(a, b):
    return [a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
            a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3], a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1]]


def qinv(q):
    n2 = sum(x * x for x in q)
    return [q[0] / n2, -q[1] / n2, -q[2] / n2, -q[3] / n2]


def rot_of(q):
    w, x, y, z = q
    return mpmath.matrix([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                          [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def iso(R, t):
    T = mpmath.eye(4)
    T[0:3, 0:3] = R; T[0:3, 3] = t
    return T


def vio_fields(v):
    return dict(ti=mpf(v[0]), tj=mpf(v[1]), tl=mpf(v[2]), Ri=M(v[3:12], 3, 3), Pi=M(v[12:15], 3, 1), Vi=M(v[15:18], 3, 1), Rj=M(v[18:27], 3, 3), Pj=M(v[27:30], 3, 1),
                Vj=M(v[30:33], 3, 1))


def ref_motion(v, step, RLB, TLB):
    f = vio_fields(v); step = mpf(step)
    tls, tle = f["tl"] - step / 2, f["tl"] + step / 2
    qa, qb = quat_of(f["Ri"]), quat_of(f["Rj"])
    ss, se = (tls - f["ti"]) / (f["tj"] - f["ti"]), (tle - f["ti"]) / (f["tj"] - f["ti"])
    qls, qle = slerp(qa, ss, qb), slerp(qa, se, qb)
    Rb = rot_of(qmul(qinv(qle), qls))
    tb = (-f["Rj"].T * f["Pj"] + f["Rj"].T * f["Pi"]) * step / (f["tj"] - f["ti"])
    Tlb = iso(M(RLB, 3, 3), M(TLB, 3, 1))
    Tl = Tlb * iso(Rb, tb) * Tlb ** -1
    return Tl, tls, tle, qls, qle


def ref_predict(vi, vj, RLB, TLB, TBL):
    def r_of(f):
        t = (f["tl"] - f["ti"]) / (f["tj"] - f["ti"])
        qa, qb = quat_of(f["Ri"]), quat_of(f["Rj"])
        return rot_of(slerp(qa, t, qb) if t > 0 else qa)                 # q.normalized() is discarded

    def t_of(f):
        dt = f["tl"] - f["ti"]
        if dt >= 0:
            a = (f["Vj"] - f["Vi"]) / (f["tj"] - f["ti"])
            return f["Pi"] + f["Vi"] * dt + a * dt * dt / 2
        return f["Pi"]
    fi, fj = vio_fields(vi), vio_fields(vj)
    RLB, TLB, TBL = M(RLB, 3, 3), M(TLB, 3, 1), M(TBL, 3, 1)
    RBL = RLB.T
    Rbj, Rbi, Tbj, Tbi = r_of(fj), r_of(fi), t_of(fj), t_of(fi)
    Rij = Rbi ** -1 * Rbj
    Tij = Rbi.T * Tbj - Rbi.T * Tbi
    guess = iso(RLB * Rij * RLB.T, RLB * Rij * TBL + TLB + RLB * Tij)
    return iso(Rij, Tij), guess, Rbi * RBL, Tbi + Rbi * TBL, Rbj * RBL, Tbj + Rbj * TBL


def flat(Mx):
    return [Mx[i, j] for i in range(Mx.rows) for j in range(Mx.cols)]


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    return np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])


def vio(ti, tj, tl, Ri, Pi, Vi, Rj, Pj, Vj):
    return [ti, tj, tl] + list(np.ravel(Ri)) + list(Pi) + list(Vi) + list(np.ravel(Rj)) + list(Pj) + list(Vj)


RLB = rot(0.01, -0.02, 1.55); TLB = np.array([0.05, -0.02, 0.12]); TBL = -RLB.T @ TLB
RA = rot(0.02, -0.01, 0.4)
VIOS = {
    "generic": vio(10.0, 10.1, 10.04, RA, [1.0, 2.0, 0.3], [0.5, -0.2, 0.01], RA @ rot(0.004, -0.003, 0.02), [1.05, 1.98, 0.301], [0.52, -0.19, 0.0]),
    "same_rotation": vio(10.0, 10.1, 10.06, RA, [1.0, 2.0, 0.3], [0.5, -0.2, 0.01], RA, [1.05, 1.98, 0.301], [0.5, -0.2, 0.01]),              # absD >= 1 - eps
    "half_turn": vio(20.0, 20.1, 20.05, rot(0, 0, 2.0), [0, 0, 0], [0.1, 0, 0], rot(0, 0, -2.0), [0.01, 0, 0], [0.1, 0, 0]),                  # d < 0: the sign flip
    "scan_before_left": vio(30.0, 30.1, 29.98, RA, [1.0, 2.0, 0.3], [0.5, -0.2, 0.01], RA @ rot(0.01, 0, 0.03), [1.05, 1.98, 0.3], [0.4, -0.1, 0]),      # t <= 0, dt < 0
    "pitch_up": vio(40.0, 40.1, 40.03, rot(0, 2.9, 0), [0, 1, 0], [0, 0.3, 0], rot(0.01, 2.92, 0), [0, 1.03, 0], [0, 0.31, 0]),               # trace < 0, largest diagonal entry: y
}
# |entries| <= 1 for rotations, a few units for positions: each double operation rounds by at most half an ulp of a value of magnitude S,
# the paths are 100-200 operations long, acos amplifies its argument's rounding by 1 / sin(theta) and the scale factors take it back
# (d scale / d theta = O(theta)): 1024 ulp(S) bounds a faithful restatement, a wrong branch or order errs by the rotation angle (>= 1e-3).
TOL = 1024 * EPS64


def close(got, want, scale):
    return all(abs(mpf(g) - w) <= TOL * scale for g, w in zip(got, want))


@pytest.mark.parametrize("name", sorted(VIOS))
def test_deskew_motion(exe, name):
    v = VIOS[name]
    (tag, out), = run(exe, [("M", v + [0.1] + list(RLB.ravel()) + list(TLB))])
    assert tag == "M" and out[0] == 1
    q, t, tf, tls, tle = out[1:5], out[5:8], out[8], out[9], out[10]
    Tl, rtls, rtle, qls, qle = ref_motion(v, 0.1, RLB.ravel(), TLB)
    assert tf == float(np.float32(1 / 0.1)) and tls == v[2] - 0.5 * 0.1 and tle == v[2] + 0.5 * 0.1
    # the float translation and the float quaternion: the double result rounded once, so within one float ulp (and the double path's error)
    f32 = float(np.finfo(np.float32).eps)
    for k in range(3):
        assert abs(mpf(t[k]) - Tl[k, 3]) <= f32 * abs(Tl[k, 3]) + TOL, (k, t[k], Tl[k, 3])
    qr = quat_of(Tl[0:3, 0:3])
    sign = 1 if sum(mpf(a) * b for a, b in zip(q, qr)) >= 0 else -1
    assert all(abs(mpf(a) * sign - b) <= 8 * f32 for a, b in zip(q, qr)), (q, qr)              # the conversion runs in float: ~10 operations on a rounded matrix
    assert abs(sum(a * a for a in q) - 1) <= 8 * f32
    if name == "same_rotation":
        assert abs(sum(x * y for x, y in zip(quat_of(M(v[3:12], 3, 3)), quat_of(M(v[18:27], 3, 3))))) >= 1 - mpf(EPS64)
    if name == "half_turn":
        qa, qb = quat_of(M(v[3:12], 3, 3)), quat_of(M(v[18:27], 3, 3))
        assert sum(x * y for x, y in zip(qa, qb)) < 0
    if name == "pitch_up":
        assert v[3] + v[7] + v[11] < 0 and v[7] > v[3] and v[7] > v[11]                                # no positive trace: the branch by the largest diagonal entry


@pytest.mark.parametrize("pair", [("generic", "same_rotation"), ("scan_before_left", "generic"), ("half_turn", "pitch_up"), ("same_rotation", "scan_before_left")])
def test_predict_relative(exe, pair):
    vi, vj = VIOS[pair[0]], VIOS[pair[1]]
    (tag, out), = run(exe, [("P", vi + vj + list(RLB.ravel()) + list(TLB) + list(TBL))])
    assert tag == "P" and out[0] == 1
    Lij, guess, Ri, Ti, Rj, Tj = ref_predict(vi, vj, RLB.ravel(), TLB, TBL)
    want = flat(Lij) + flat(guess) + flat(Ri) + flat(Ti) + flat(Rj) + flat(Tj)
    assert len(out) - 1 == len(want) == 16 + 16 + 9 + 3 + 9 + 3
    scale = 1 + max(abs(w) for w in want)
    worst = max(abs(mpf(g) - w) for g, w in zip(out[1:], want)) / scale
    print(pair, "worst error", float(worst / EPS64), "ulp(S)")
    assert close(out[1:], want, scale)
    if "scan_before_left" in pair:                               # t <= 0 and dt < 0: the left keyframe's pose as it is
        k = pair.index("scan_before_left")
        v = VIOS["scan_before_left"]
        assert v[2] < v[0]
        R = [Ri, Rj][k]; T = [Ti, Tj][k]
        assert close(flat(R), flat(M(v[3:12], 3, 3) * M(RLB.ravel(), 3, 3).T), 2) and close(flat(T), flat(M(v[12:15], 3, 1) + M(v[3:12], 3, 3) * M(TBL, 3, 1)), 4)


# ---- the deque --------------------------------------------------------------------------------------------------------------------------
class PyQueue:
    """estimator.cpp:378-435 in plain Python"""

    def __init__(self):
        self.q, self.first_zv, self.zv = [], True, None

    def push(self, mode, applied, ti, tj, Ri, Ti, cur):
        e = (mode, applied, ti[0], ti[1], tj[0], tj[1], ti[2], tj[2])
        if applied == 4:
            if self.first_zv:
                self.zv = cur = (list(Ri), list(Ti)); self.first_zv = False
                while len(self.q) > 1:
                    self.q.pop(0)
            else:
                cur = self.zv
        elif applied == 3:
            if not self.first_zv and len(self.q) == 1:
                self.q.pop(0); self.first_zv = True
        self.q.append(e)
        return cur


def test_constraint_queue_walks_the_mode_sequence(exe):
    """Moving, moving, zero velocity for the first time, zero velocity again (twice), moving again, pure rotation, then the ADD_LIDAR_ICP = 0
    override (mode 4 classified, 0 applied) and a second stop: the deque and the carried lidar_R / lidar_T after every step."""
    modes = [(3, 3), (3, 3), (2, 2), (4, 4), (4, 4), (4, 4), (3, 3), (5, 5), (4, 0), (3, 3), (4, 4), (1, 1), (4, 4)]
    rng = np.random.default_rng(3)
    lines, py, want = [], PyQueue(), []
    for k, (mode, applied) in enumerate(modes):
        ti, tj = [100.0 + k, 100.05 + k, 100.02 + k], [101.0 + k, 101.05 + k, 101.02 + k]
        Ri, Ti, Rc, Tc = rng.normal(size=9), rng.normal(size=3), rng.normal(size=9), rng.normal(size=3)
        lines.append(("Q", [mode, applied] + ti + tj + list(Ri) + list(Ti) + list(Rc) + list(Tc)))
        cur = py.push(mode, applied, ti, tj, Ri, Ti, (list(Rc), list(Tc)))
        want.append([len(py.q), int(py.first_zv)] + list(cur[0]) + list(cur[1]) + [float(v) for e in py.q for v in e])
    got = run(exe, lines)
    assert len(got) == len(want)
    for k, ((tag, out), w) in enumerate(zip(got, want)):
        assert tag == "Q" and out == w, (k, modes[k], out[:2], w[:2])
    sizes = [w[0] for w in want]; first = [w[1] for w in want]
    # moving grows the deque; the first stop cuts it to one and adds itself; later stops add; moving again with exactly one entry pops it
    assert sizes[:6] == [1, 2, 3, 2, 3, 4] and first[:6] == [1, 1, 1, 0, 0, 0]
    assert sizes[6] == 5 and first[6] == 0                       # four entries, not one: "start moving again" does not fire
    assert first[8] == 0 and first[9] == 0
    # a stop that finds first_zv set trims to one entry; the next moving pair then finds two entries and does not pop
    q2 = PyQueue()
    for step in [(3, 3), (4, 4), (3, 3)]:
        q2.push(step[0], step[1], [0, 0, 0], [0, 0, 0], [0] * 9, [0] * 3, ([0] * 9, [0] * 3))
    assert len(q2.q) == 3 and q2.first_zv is False
    q3 = PyQueue()
    for step in [(4, 4), (3, 3)]:                                  # a stop on an empty deque, then moving: the one entry is popped
        q3.push(step[0], step[1], [0, 0, 0], [0, 0, 0], [0] * 9, [0] * 3, ([0] * 9, [0] * 3))
    assert len(q3.q) == 1 and q3.first_zv is True and q3.q[0][0] == 3


def test_start_moving_again_pops_the_single_entry(exe):
    z9, z3 = [0.0] * 9, [0.0] * 3
    lines = [("Q", [4, 4, 1, 2, 3, 4, 5, 6] + [1.0] * 9 + [2.0] * 3 + z9 + z3), ("Q", [3, 3, 7, 8, 9, 10, 11, 12] + z9 + z3 + [5.0] * 9 + [6.0] * 3),
             ("Q", [4, 4, 13, 14, 15, 16, 17, 18] + [7.0] * 9 + [8.0] * 3 + z9 + z3)]
    got = run(exe, lines)
    assert got[0][1][:2] == [1, 0] and got[0][1][2:14] == [1.0] * 9 + [2.0] * 3                      # first stop: frame i's pose is carried
    assert got[1][1][:2] == [1, 1] and got[1][1][2:14] == [5.0] * 9 + [6.0] * 3                      # moving again: popped, first_zv set, pose untouched
    assert got[1][1][14:22] == [3, 3, 7, 8, 10, 11, 9, 12]                                           # ta tb tc td ti tj
    assert got[2][1][:2] == [2, 0] and got[2][1][2:14] == [7.0] * 9 + [8.0] * 3                      # a first stop again
