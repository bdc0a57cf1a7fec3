"""ctypes layer over include/villoop.h: the alignment fitness score (pcl::Registration::getFitnessScore) of a resident scan pair and the
loop-closure verification built on it (performICP / findLoopClosure of lidar_mapping).

`LoopVerify(cdll)` drives csrc/libvilsolve.so (HIP; needs a GPU, no CPU fallback).  The only CPU restatement is tests/loopverify_ref.py.
"""
import ctypes as C
import sys

import numpy as np

from ._row import RowError, RowHandle
from .vgicp import VgicpOptions

MAX_BATCH = 16
SUM_BLOCK = 256
DBL_MAX = sys.float_info.max
FLT_MAX = float(np.finfo(np.float32).max)
KERNELS = ("k_loop_grid", "k_loop_brute", "k_loop_sum", "k_loop_finish")
_FP, _DP, _IP = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32)


class VloopCandidate(C.Structure):
    _fields_ = [("n", C.c_int32), ("pad", C.c_int32), ("xyz", _FP), ("guess", C.c_double * 16)]


class VloopOptions(C.Structure):
    _fields_ = [("reg", VgicpOptions), ("resolution", C.c_double), ("max_tolerable_fitness", C.c_float), ("pad", C.c_int32)]


class VloopCandidateResult(C.Structure):
    _fields_ = [("converged", C.c_int32), ("fitness", C.c_float), ("n_used", C.c_int32), ("iterations", C.c_int32), ("T", C.c_double * 16)]


class VloopBest(C.Structure):
    _fields_ = [("index", C.c_int32), ("fitness", C.c_float), ("n_used", C.c_int32), ("pad", C.c_int32), ("T", C.c_double * 16), ("delta", C.c_double * 16)]


class LoopVerifyError(RowError):
    pass


def default_options(cdll, **kw):
    """vloop_default_options; keyword arguments set fields of vloop_options, or of its vgicp_options when they are not its own."""
    o = VloopOptions()
    f = cdll.vloop_default_options; f.restype = None
    f(C.byref(o))
    for k, v in kw.items():
        if k in dict(VloopOptions._fields_) and k != "reg":
            setattr(o, k, v)
        elif k in dict(VgicpOptions._fields_):
            setattr(o.reg, k, v)
        else:
            raise AttributeError("vloop_options has no field %r" % k)
    return o


def mat(a16):
    """A 4 x 4 float64 array from a c_double * 16."""
    return np.array(a16[:], np.float64).reshape(4, 4)


class LoopVerify(RowHandle):
    """A resident (source, target) pair and its score.  max_points bounds either cloud."""
    ERROR, KERNELS = LoopVerifyError, KERNELS

    def __init__(self, cdll, max_points=1 << 17, device=0):
        super().__init__(cdll, "vloop_")
        self.n_source = 0
        self._create(C.c_int32(device), C.c_int32(max_points))

    def set_target(self, xyz):
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        self._call("set_target", C.c_int32(len(xyz)), xyz.ctypes.data_as(_FP))

    def set_source(self, xyz):
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        self._call("set_source", C.c_int32(len(xyz)), xyz.ctypes.data_as(_FP))
        self.n_source = len(xyz)

    def set_grid(self, min_points, cell):
        self._call("set_grid", C.c_int32(min_points), C.c_double(cell))

    def score(self, T, max_range=DBL_MAX, debug=False):
        """T: 4 x 4 or n_T x 4 x 4 (source -> target).  Returns (scores float64, n_used int32), each of n_T entries (scalars for a single
        4 x 4); with debug also (nn_d2 float32, nn_idx int32), n_T x n_source each."""
        T = np.ascontiguousarray(T, np.float64)
        single = T.ndim == 2
        T = T.reshape(-1, 4, 4)
        n = len(T)
        scores = np.zeros(n, np.float64); used = np.zeros(n, np.int32)
        d2 = np.zeros((n, self.n_source), np.float32) if debug else None
        idx = np.zeros((n, self.n_source), np.int32) if debug else None
        self._call("score", C.c_int32(n), T.ctypes.data_as(_DP), C.c_double(max_range), scores.ctypes.data_as(_DP), used.ctypes.data_as(_IP),
                   d2.ctypes.data_as(_FP) if debug else C.cast(None, _FP), idx.ctypes.data_as(_IP) if debug else C.cast(None, _IP))
        out = (scores[0], used[0]) if single else (scores, used)
        if debug:
            out += (d2[0], idx[0]) if single else (d2, idx)
        return out

    def verify(self, reg, query, candidates, options=None):
        """reg: a vgicp.Vgicp on the same library.  query: n x 3.  candidates: [(xyz n x 3, guess 4 x 4)] in the order they are tried.
        Returns (VloopBest, [VloopCandidateResult])."""
        query = np.ascontiguousarray(query, np.float32).reshape(-1, 3)
        if options is None:
            options = default_options(self.lib)
        keep = [np.ascontiguousarray(x, np.float32).reshape(-1, 3) for x, _ in candidates]
        n = len(candidates)
        cs = (VloopCandidate * max(n, 1))()
        for k, (x, (_, g)) in enumerate(zip(keep, candidates)):
            cs[k].n = len(x); cs[k].xyz = x.ctypes.data_as(_FP)
            cs[k].guess[:] = [float(v) for v in np.asarray(g, np.float64).reshape(16)]
        per = (VloopCandidateResult * max(n, 1))()
        best = VloopBest()
        self._call("verify", reg.ctx, C.c_int32(len(query)), query.ctypes.data_as(_FP), C.c_int32(n), cs, C.byref(options), C.byref(best), per)
        self.n_source = len(query)
        return best, list(per[:n])
