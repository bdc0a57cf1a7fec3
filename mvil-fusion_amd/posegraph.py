"""ctypes layer over include/vilpgo.h: the resident pose graph of lidar_mapping's loop closure (prior, between and position factors over
6-dof poses) and its Levenberg-Marquardt optimisation on the device.

`PoseGraph(cdll)` drives csrc/libvilsolve.so (HIP; needs a GPU, no CPU fallback).  The only CPU restatement is tests/posegraph_ref.py.
"""
import ctypes as C

import numpy as np

from ._row import RowError, RowHandle

SEGMENT = 64
MAX_SEPARATORS = 256
SUM_BLOCK = 256
SMALL_ANGLE = 1e-4
LAMBDA_FLOOR = 1e-6
MAX_ITERATIONS = 100
PRIOR, BETWEEN, POSITION = 0, 1, 2
TERM_NONE, TERM_STEP, TERM_COST, TERM_MAX_ITERATIONS = 0, 1, 2, 3
ERR_CAPACITY = -7
KERNELS = ("k_pgo_lin", "k_pgo_gather", "k_pgo_segment", "k_pgo_schur", "k_pgo_chol", "k_pgo_dense_back", "k_pgo_seg_back", "k_pgo_update", "k_pgo_reduce",
           "k_pgo_decide", "k_pgo_finish")
_DP, _IP = C.POINTER(C.c_double), C.POINTER(C.c_int32)


class VpgoOptions(C.Structure):
    _fields_ = [("max_iterations", C.c_int32), ("pad", C.c_int32), ("initial_lambda", C.c_double), ("step_tolerance", C.c_double), ("cost_tolerance", C.c_double)]


class VpgoSummary(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("accepted", C.c_int32), ("termination", C.c_int32), ("reduced_size", C.c_int32), ("n_separators", C.c_int32),
                ("n_segments", C.c_int32), ("initial_cost", C.c_double), ("final_cost", C.c_double), ("final_lambda", C.c_double)]


class PoseGraphError(RowError):
    pass


def default_options(cdll, **kw):
    """vpgo_default_options; keyword arguments set fields of vpgo_options."""
    o = VpgoOptions()
    f = cdll.vpgo_default_options; f.restype = None
    f(C.byref(o))
    for k, v in kw.items():
        if k not in dict(VpgoOptions._fields_):
            raise AttributeError("vpgo_options has no field %r" % k)
        setattr(o, k, v)
    return o


def _d(a, n):
    a = np.ascontiguousarray(a, np.float64).reshape(-1)
    if a.size != n:
        raise ValueError("expected %d doubles, got %d" % (n, a.size))
    return a


class PoseGraph(RowHandle):
    """A resident pose graph.  Poses and measurements are 4 x 4 arrays, variances are 6 (rotation first) or 3 long."""
    ERROR, KERNELS = PoseGraphError, KERNELS

    def __init__(self, cdll, max_poses=1 << 14, max_factors=1 << 15, device=0):
        super().__init__(cdll, "vpgo_")
        self._create(C.c_int32(device), C.c_int32(max_poses), C.c_int32(max_factors))

    def add_pose(self, T):
        key = C.c_int32(-1)
        self._call("add_pose", _d(T, 16).ctypes.data_as(_DP), C.byref(key))
        return key.value

    def add_prior(self, i, Z, var6):
        self._call("add_prior", C.c_int32(i), _d(Z, 16).ctypes.data_as(_DP), _d(var6, 6).ctypes.data_as(_DP))

    def add_between(self, i, j, Z, var6):
        self._call("add_between", C.c_int32(i), C.c_int32(j), _d(Z, 16).ctypes.data_as(_DP), _d(var6, 6).ctypes.data_as(_DP))

    def add_position(self, i, z, var3):
        self._call("add_position", C.c_int32(i), _d(z, 3).ctypes.data_as(_DP), _d(var3, 3).ctypes.data_as(_DP))

    def size(self):
        """(poses, factors, separators)"""
        n = (C.c_int32 * 3)()
        self._call("size", C.byref(n, 0), C.byref(n, 4), C.byref(n, 8))
        return n[0], n[1], n[2]

    def optimize(self, options=None, **kw):
        if options is None:
            options = default_options(self.lib, **kw)
        sm = VpgoSummary()
        self._call("optimize", C.byref(options), C.byref(sm))
        return sm

    def poses(self, first=0, n=None):
        """n x 4 x 4"""
        if n is None:
            n = self.size()[0] - first
        out = np.zeros((n, 4, 4), np.float64)
        self._call("get_poses", C.c_int32(first), C.c_int32(n), out.ctypes.data_as(_DP))
        return out

    def relative(self, i, j):
        """T_j^-1 T_i"""
        out = np.zeros((4, 4), np.float64)
        self._call("relative", C.c_int32(i), C.c_int32(j), out.ctypes.data_as(_DP))
        return out

    def step(self):
        """N x 6: the step the last attempt of the last optimize solved for"""
        d = np.zeros((self.size()[0], 6))
        self._call("get_step", d.ctypes.data_as(_DP))
        return d

    def eval(self):
        """(r F x 6, J_i F x 6 x 6, J_j F x 6 x 6, cost, g N x 6) at the current state"""
        N, F, _ = self.size()
        r = np.zeros((F, 6)); Ji = np.zeros((F, 6, 6)); Jj = np.zeros((F, 6, 6)); g = np.zeros((N, 6)); cost = C.c_double(0.0)
        self._call("eval", r.ctypes.data_as(_DP), Ji.ctypes.data_as(_DP), Jj.ctypes.data_as(_DP), C.byref(cost), g.ctypes.data_as(_DP))
        return r, Ji, Jj, cost.value, g
