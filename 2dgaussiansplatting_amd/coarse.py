"""CoarseTrainer: coarse-to-fine fitting (include/splat2d_coarse.h) on top of Trainer -- the context's target seen through a
view's window, and whole training iterations at a view's size.

The two entry points are declared in a header of their own, so their signatures stand here, in a table of this module's, and
are applied to the library a trainer was created with.  No torch: device buffers cross as addresses."""
import ctypes as C

import numpy as np

from ._abi import S2D_E_INVALID, S2D_STEP_OPTIMIZE_OPACITY, _ViewConfig
from ._handle import S2DError, _p
from .trainer import Trainer, _dev

_vp, _i32, _u32, _int = C.c_void_p, C.c_int32, C.c_uint32, C.c_int

# name -> (argtypes, restype) of the symbols include/splat2d_coarse.h declares, in its order
COARSE_SIGNATURES = {
    "s2d_view_target_device": ([_vp, C.POINTER(_ViewConfig), _vp], _int),
    "s2d_step_view": ([_vp, C.POINTER(_ViewConfig), _vp, _i32, _u32, _vp], _int),
}
COARSE_SYMBOLS = list(COARSE_SIGNATURES)


def apply_coarse_signatures(L):
    """Sets argtypes and restype of the two symbols on the loaded library L; a library without them raises AttributeError."""
    for name, (argtypes, restype) in COARSE_SIGNATURES.items():
        f = getattr(L, name)
        f.argtypes, f.restype = argtypes, restype


class CoarseTrainer(Trainer):
    """A Trainer that can also train at a view's size (s2d_step_view) and resample its target to a view's window
    (s2d_view_target_device).  Everything else is Trainer's."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        apply_coarse_signatures(self.L)

    def view_target_device(self, ptr, out_width, out_height, origin=(0.0, 0.0), zoom=1.0):
        """The target seen through the window into device memory at `ptr` (out_height x out_width RGBA32F, 16-byte aligned),
        queued on the context's stream: the box resample of include/splat2d_coarse.h."""
        cfg = self._view_config(out_width, out_height, origin, zoom)
        self._ck(self.L.s2d_view_target_device(self._h, C.byref(cfg), _dev(ptr)))

    def view_target(self, out_width, out_height, origin=(0.0, 0.0), zoom=1.0):
        """The same as an (out_height, out_width, 4) float32 array on the host."""
        hip = self._hip()
        self.synchronize()  # (also makes the context's device this thread's current one: the buffer must live there)
        a = np.zeros((int(out_height), int(out_width), 4), dtype=np.float32)
        buf = C.c_void_p()
        if hip.hipMalloc(C.byref(buf), C.c_size_t(max(a.nbytes, 16))) != 0:
            raise MemoryError("hipMalloc of %d bytes for the view's target failed" % a.nbytes)
        try:
            self.view_target_device(buf.value, out_width, out_height, origin, zoom)
            self.synchronize()
            if hip.hipMemcpy(_p(a), buf, C.c_size_t(a.nbytes), 2) != 0:  # hipMemcpyDeviceToHost
                raise RuntimeError("hipMemcpy of the view's target failed")
        finally:
            hip.hipFree(buf)
        return a

    def step_view(self, iters, out_width, out_height, origin=(0.0, 0.0), zoom=1.0, filter_var=0.0, samples=1, target_ptr=0,
                  optimize_opacity=False):
        """iters iterations at the view's size (s2d_step_view) against the target at `target_ptr` (device, out_height x
        out_width RGBA32F, 16-byte aligned) or, with 0, the library's own resample of the context's target; returns the MSE of
        the view before each step.  optimize_opacity: S2D_STEP_OPTIMIZE_OPACITY."""
        if int(iters) < 0:
            raise S2DError(S2D_E_INVALID, "step_view: iters < 0")
        cfg = self._view_config(out_width, out_height, origin, zoom, filter_var, samples)
        out = np.zeros(int(iters), dtype=np.float64)
        flags = S2D_STEP_OPTIMIZE_OPACITY if optimize_opacity else 0
        self._ck(self.L.s2d_step_view(self._h, C.byref(cfg), _dev(target_ptr), int(iters), flags, _p(out)))
        return out

    def _hip(self):
        """The HIP runtime the library is linked against (the one mapped into this process)."""
        from ._runtime import hip_runtimes_mapped
        paths = hip_runtimes_mapped()
        if not paths:
            raise RuntimeError("no HIP runtime is mapped into this process")
        hip = C.CDLL(paths[0])
        hip.hipMalloc.argtypes, hip.hipMalloc.restype = [C.POINTER(C.c_void_p), C.c_size_t], C.c_int
        hip.hipMemcpy.argtypes, hip.hipMemcpy.restype = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], C.c_int
        hip.hipFree.argtypes, hip.hipFree.restype = [C.c_void_p], C.c_int
        return hip
