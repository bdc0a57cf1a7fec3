"""The ctypes handle the row wrappers share (scanreg, depthreg, scancontext, loopverify, mapreg, vgicp, preint, track, epipolar, clahe, feat, cloud, lidarfront, localmap): one context behind one C prefix,
a status check on every call, close / __del__, and the kernel profiler of the rows that have one."""
import ctypes as C


class RowError(RuntimeError):
    """A row call that returned a non-zero status; `status` is that code (None when raised with a bare message)."""

    def __init__(self, message, status=None):
        super().__init__(message)
        self.status = status


class RowHandle:
    """lib: the CDLL.  prefix: the row's C prefix ("vscan_", "orc_vmap_").  ctx: the row's context (c_void_p), None after close() or a
    failed create.  A subclass names its error class in ERROR and the kernels its X_profile_read reports in KERNELS, in the order of
    the C arrays: the library writes one count and one time per kernel, so without KERNELS there is no profile_read."""
    ERROR = RowError
    KERNELS = ()

    def __init__(self, cdll, prefix):
        self.lib, self.prefix = cdll, prefix
        self.ctx = None
        self._fcache = {}

    def _f(self, name):
        f = self._fcache.get(name)
        if f is None:
            f = getattr(self.lib, self.prefix + name)
            f.restype = C.c_int
            self._fcache[name] = f
        return f

    def _chk(self, name, st, hint=""):
        if st != 0:
            raise self.ERROR("%s%s failed: status %d%s" % (self.prefix, name, st, hint), st)

    def _create(self, *args, hint=""):
        """X_create(*args, &ctx)"""
        ctx = C.c_void_p()
        self._chk("create", self._f("create")(*args, C.byref(ctx)), hint)
        self.ctx = ctx

    def _call(self, name, *args):
        """X_name(ctx, *args)"""
        self._chk(name, self._f(name)(self.ctx, *args))

    def close(self):
        if getattr(self, "ctx", None) is not None:
            f = getattr(self.lib, self.prefix + "destroy"); f.restype = None
            f(self.ctx); self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def profile_enable(self, on=True):
        self._call("profile_enable", C.c_int32(1 if on else 0))

    def profile_read(self):
        """{kernel: (launches, total ms)} since the last read."""
        if not self.KERNELS:
            raise TypeError("%s names no KERNELS: the arrays for %sprofile_read cannot be sized" % (type(self).__name__, self.prefix))
        n = (C.c_int64 * len(self.KERNELS))(); ms = (C.c_double * len(self.KERNELS))()
        self._call("profile_read", n, ms)
        return {k: (int(n[i]), float(ms[i])) for i, k in enumerate(self.KERNELS)}
