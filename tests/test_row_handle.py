"""The ctypes handle the row wrappers share (mvil-fusion_amd/_row.py), driven through a fake library: no GPU, no shared object."""
import pytest

from mvil_fusion_amd import _row, depthreg, mapreg, preint, scancontext, scanreg, vgicp


class FakeError(_row.RowError):
    pass


class FakeLib:
    """vfake_* entry points that return the scripted statuses and record what was called."""

    def __init__(self, **status):
        self.status, self.calls = status, []
        for name in ("create", "destroy", "profile_enable", "profile_read", "work"):
            setattr(self, "vfake_" + name, self._entry(name))

    def _entry(self, name):
        def f(*args):
            self.calls.append(name)
            if name == "create" and self.status.get("create", 0) == 0:
                args[-1]._obj.value = 0x1234                                  # byref(ctx)
            if name == "profile_read":
                ctx, n, ms = args
                for i in range(len(n)):
                    n[i] = 10 * (i + 1); ms[i] = 0.5 * (i + 1)
            return self.status.get(name, 0)
        return f


class Fake(_row.RowHandle):
    ERROR, KERNELS = FakeError, ("k_a", "k_b", "k_c")

    def __init__(self, lib):
        super().__init__(lib, "vfake_")
        self._create()


def test_failed_create_raises_and_is_never_destroyed():
    lib = FakeLib(create=-2)
    with pytest.raises(FakeError) as e:
        Fake(lib)
    assert e.value.status == -2 and str(e.value) == "vfake_create failed: status -2"
    h = Fake.__new__(Fake); _row.RowHandle.__init__(h, lib, "vfake_")
    with pytest.raises(FakeError):
        h._create()
    assert h.ctx is None
    h.close(); h.__del__()
    assert "destroy" not in lib.calls


def test_close_destroys_exactly_once():
    lib = FakeLib()
    h = Fake(lib)
    assert h.ctx.value == 0x1234 and h.lib is lib and h.prefix == "vfake_"
    h.close(); h.close(); h.__del__()
    assert h.ctx is None and lib.calls.count("destroy") == 1


def test_non_zero_status_of_a_call_raises_with_the_old_message():
    lib = FakeLib(work=-2)
    h = Fake(lib)
    with pytest.raises(FakeError) as e:
        h._call("work", 1, 2)
    assert str(e.value) == "vfake_work failed: status -2" and e.value.status == -2
    lib.status["work"] = 0
    h._call("work")
    h.close()


def test_profile_read_is_keyed_by_kernels_in_order():
    lib = FakeLib()
    h = Fake(lib)
    h.profile_enable(True)
    prof = h.profile_read()
    assert list(prof) == ["k_a", "k_b", "k_c"]
    assert prof == {"k_a": (10, 0.5), "k_b": (20, 1.0), "k_c": (30, 1.5)}
    assert all(type(n) is int and type(ms) is float for n, ms in prof.values())
    lib.status["profile_read"] = -1
    with pytest.raises(FakeError) as e:
        h.profile_read()
    assert e.value.status == -1
    h.close()


def test_the_six_error_classes_keep_their_names_and_status():
    for cls in (scanreg.ScanRegError, depthreg.DepthRegError, scancontext.ScanContextError, mapreg.MapRegError, vgicp.VgicpError, preint.PreintError):
        assert issubclass(cls, RuntimeError)
        assert cls("x_y failed: status -6", -6).status == -6
    for row, cls in ((scanreg.ScanReg, scanreg.ScanRegError), (depthreg.DepthReg, depthreg.DepthRegError), (scancontext.ScanContext, scancontext.ScanContextError),
                     (mapreg.MapReg, mapreg.MapRegError), (vgicp.Vgicp, vgicp.VgicpError), (preint.Preint, preint.PreintError)):
        assert row.ERROR is cls


def test_profile_read_needs_kernels():
    """X_profile_read writes one count and one time per kernel: a handle without KERNELS must not hand it empty arrays."""
    class Bare(_row.RowHandle):
        ERROR = FakeError
    lib = FakeLib()
    h = Bare(lib, "vfake_"); h._create()
    with pytest.raises(TypeError):
        h.profile_read()
    assert "profile_read" not in lib.calls
    h.close()
    assert mapreg.MapReg.KERNELS == ("k_map_search", "k_map_fit") and vgicp.Vgicp.KERNELS == ("k_vgicp_lin",) and preint.Preint.KERNELS == ("k_preint",)
    assert scanreg.ScanReg.KERNELS == scanreg.KERNELS and depthreg.DepthReg.KERNELS == depthreg.KERNELS and scancontext.ScanContext.KERNELS == scancontext.KERNELS
