"""The host-timed max_time_s cap of the chunked launch structures (csrc/vilsolve.hip, solve_attempt): one launch per iteration (k_iter, launch mode 4) and
two launches per iteration (sweep + gather / step, launch mode 3).  The host reads its clock between two chunks of enqueued iterations and ends the solve
with the accepted state of the chunk's last iteration (include/vilsolve.h, vil_options.max_time_s); test_gpu_persist.py covers the device-read cap of k_solve."""
import copy
import ctypes as C

import numpy as np
import pytest

from mvil_fusion_amd import abi, lib, synth

pytestmark = pytest.mark.gpu


def bits(s):
    return (s.iterations, s.successful_steps, s.termination, float(s.initial_cost).hex(), float(s.final_cost).hex(),
            [float(v).hex() for v in list(s.cost_trace)[:s.iterations]])


def state_of(be, w):
    w = copy.deepcopy(w)
    be.download_state(w)
    return np.concatenate([w.pose.ravel(), w.speedbias.ravel(), w.ex_pose.ravel(), w.td.ravel(), w.inv_depth.ravel()])


@pytest.fixture(scope="module")
def window(oracle):
    w = synth.make_config(2, L=120, n_plane=1000, n_edge=333)
    assert oracle.solve(copy.deepcopy(w)).iterations >= 6          # (13: the capped solve's one chunk of three iterations cannot finish it)
    return w


@pytest.mark.parametrize("mode,launches", [(4, 1), (3, 2)])
def test_host_timed_cap_ends_a_chunked_solve_at_a_chunk_boundary(window, mode, launches):
    be = lib.open_vilsolve()
    try:
        assert be.lib.vil_debug_set_launch_mode(be.ctx, mode) == 0
        be.upload(window)
        n, one = C.c_int32(-1), C.c_int32(-1)
        assert be.lib.vil_debug_get_launch_structure(be.ctx, C.byref(n), C.byref(one)) == 0
        assert n.value == launches
        s_full = be.solve_resident(); x_full = state_of(be, window)
        print("mode %d: un-capped %d iterations, cost %.17g -> %.17g" % (mode, s_full.iterations, s_full.initial_cost, s_full.final_cost))
        assert s_full.iterations >= 6 and s_full.termination != abi.TERM_NAMES.index("max_time")
        # a solve that ends in its first iteration: the next solve's first chunk has the minimal length, three iterations
        be.reset_state(); s1 = be.solve_resident(abi.default_options(max_iterations=1))
        assert s1.termination == abi.TERM_NAMES.index("max_iterations")
        # a cap that has expired when the host reads its clock behind the first chunk
        be.reset_state(); s = be.solve_resident(abi.default_options(max_time_s=1e-7))
        tr = np.array([s_full.initial_cost] + list(s_full.cost_trace)[:s_full.iterations])
        print("mode %d: capped %d iterations, termination %s, cost %.17g, nearest entry of the un-capped trace %.3e away (relative)" %
              (mode, s.iterations, abi.TERM_NAMES[s.termination], s.final_cost, np.abs(tr - s.final_cost).min() / s.final_cost))
        assert s.termination == abi.TERM_NAMES.index("max_time")
        assert s.iterations < s_full.iterations
        assert np.abs(tr - s.final_cost).min() <= 1e-12 * s.final_cost          # an iterate of the un-capped trajectory
        # the next solve is un-capped again, and the same solve bit for bit
        be.reset_state(); s2 = be.solve_resident()
        assert bits(s2) == bits(s_full) and np.array_equal(state_of(be, window), x_full)
    finally:
        be.close()
