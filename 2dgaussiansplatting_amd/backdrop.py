"""BackdropTrainer: a backdrop behind the splats (include/splat2d_backdrop.h) on top of Trainer -- image0 = C + T_final * B for a
constant colour or an image of the context's size, the throughput plane T_final, and the gradient of the backdrop.

The five entry points are declared in a header of their own, so their signatures stand here, in a table of this module's, and
are applied to the library a trainer was created with.  No torch: device buffers cross as addresses (torch_backdrop wraps them)."""
import ctypes as C

import numpy as np

from ._abi import S2D_E_INVALID
from ._handle import S2DError, _p
from .trainer import Trainer, _dev

_vp, _int = C.c_void_p, C.c_int

# name -> (argtypes, restype) of the symbols include/splat2d_backdrop.h declares, in its order
BACKDROP_SIGNATURES = {
    "s2d_set_backdrop": ([_vp, _vp], _int),
    "s2d_set_backdrop_device": ([_vp, _vp], _int),
    "s2d_get_backdrop": ([_vp, _vp, _vp], _int),
    "s2d_throughput_device": ([_vp, _vp], _int),
    "s2d_backdrop_grads": ([_vp, _vp, _vp, _vp], _int),
}
BACKDROP_SYMBOLS = list(BACKDROP_SIGNATURES)
BACKDROP_KINDS = ("none", "constant", "plane")  # s2d_get_backdrop's kind 0, 1, 2


def apply_backdrop_signatures(L):
    """Sets argtypes and restype of the five symbols on the loaded library L; a library without them raises AttributeError."""
    for name, (argtypes, restype) in BACKDROP_SIGNATURES.items():
        f = getattr(L, name)
        f.argtypes, f.restype = argtypes, restype


class BackdropTrainer(Trainer):
    """A Trainer whose image is composited over a backdrop.  Everything else is Trainer's: while a backdrop is set, step(),
    forward_backward() and step_loss() run the separate launches and train the splats through the composite."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        apply_backdrop_signatures(self.L)

    @staticmethod
    def of(trainer):
        """`trainer` (a Trainer, e.g. the one a SplatRenderer created) as a BackdropTrainer of the same context."""
        apply_backdrop_signatures(trainer.L)
        trainer.__class__ = BackdropTrainer
        return trainer

    def set_backdrop(self, rgb):
        """A constant backdrop (r, g, b); None removes a backdrop of either kind (s2d_set_backdrop)."""
        if rgb is None:
            self._ck(self.L.s2d_set_backdrop(self._h, None))
            return
        a = np.ascontiguousarray(rgb, dtype=np.float32)
        if a.shape != (3,):
            raise S2DError(S2D_E_INVALID, "set_backdrop: three values (r, g, b), or None")
        self._ck(self.L.s2d_set_backdrop(self._h, _p(a)))

    def set_backdrop_device(self, ptr):
        """A plane backdrop from device memory at `ptr` (H x W RGBA32F, 16-byte aligned, .w ignored), copied on the context's stream
        (s2d_set_backdrop_device)."""
        self._ck(self.L.s2d_set_backdrop_device(self._h, _dev(ptr)))

    def backdrop(self):
        """-> (kind, rgb): kind "none", "constant" or "plane"; rgb the constant as three float32, zeros otherwise."""
        kind, rgb = C.c_int(), np.zeros(3, dtype=np.float32)
        self._ck(self.L.s2d_get_backdrop(self._h, C.byref(kind), _p(rgb)))
        return BACKDROP_KINDS[kind.value], rgb

    def throughput_device(self, ptr):
        """T_final of the last forward pass into device memory at `ptr` (H x W float32), queued (s2d_throughput_device)."""
        self._ck(self.L.s2d_throughput_device(self._h, _dev(ptr)))

    def throughput(self):
        """The same as an (H, W) float32 array on the host."""
        a = np.zeros((self.H, self.W), dtype=np.float32)
        self._through_device(a.nbytes, lambda buf: self.throughput_device(buf), a)
        return a

    def backdrop_grads(self, upstream_ptr=0, dplane_ptr=0, want_rgb=True):
        """dL/dB (s2d_backdrop_grads).  upstream_ptr: dL/d(image0) in device memory (H x W RGBA32F, 16-byte aligned) or 0 = image0 -
        target; dplane_ptr: where the plane's gradient (H x W RGBA32F, .w = 0) goes, or 0; want_rgb: return the three sums over the
        image as float64 (waits for the stream), otherwise None."""
        rgb = np.zeros(3, dtype=np.float64) if want_rgb else None
        self._ck(self.L.s2d_backdrop_grads(self._h, _dev(upstream_ptr), _dev(dplane_ptr), _p(rgb) if want_rgb else None))
        return rgb

    def backdrop_plane_grads(self, upstream=None):
        """Host convenience: -> (dplane (H, W, 4) float32, rgb float64[3]) for `upstream` (an (H, W, 4) float32 array, or None =
        image0 - target)."""
        hip = self._hip()
        self.synchronize()
        nbytes = self.H * self.W * 16
        bufs = [C.c_void_p(), C.c_void_p()]
        try:
            for b in bufs:
                if hip.hipMalloc(C.byref(b), C.c_size_t(max(nbytes, 16))) != 0:
                    raise MemoryError("hipMalloc of %d bytes failed" % nbytes)
            if upstream is not None:
                u = np.ascontiguousarray(upstream, dtype=np.float32)
                assert u.shape == (self.H, self.W, 4), u.shape
                if hip.hipMemcpy(bufs[0], _p(u), C.c_size_t(nbytes), 1) != 0:  # hipMemcpyHostToDevice
                    raise RuntimeError("hipMemcpy of the image gradient failed")
            rgb = self.backdrop_grads(bufs[0].value if upstream is not None else 0, bufs[1].value)
            out = np.zeros((self.H, self.W, 4), dtype=np.float32)
            if hip.hipMemcpy(_p(out), bufs[1], C.c_size_t(nbytes), 2) != 0:  # hipMemcpyDeviceToHost
                raise RuntimeError("hipMemcpy of the plane's gradient failed")
        finally:
            for b in bufs:
                if b:
                    hip.hipFree(b)
        return out, rgb

    def set_backdrop_plane(self, rgba32f):
        """Host convenience: a plane backdrop from an (H, W, 4) float32 array (uploaded, then set_backdrop_device)."""
        a = np.ascontiguousarray(rgba32f, dtype=np.float32)
        assert a.shape == (self.H, self.W, 4), a.shape
        hip = self._hip()
        self.synchronize()
        buf = C.c_void_p()
        if hip.hipMalloc(C.byref(buf), C.c_size_t(max(a.nbytes, 16))) != 0:
            raise MemoryError("hipMalloc of %d bytes for the backdrop failed" % a.nbytes)
        try:
            if hip.hipMemcpy(buf, _p(a), C.c_size_t(a.nbytes), 1) != 0:  # hipMemcpyHostToDevice
                raise RuntimeError("hipMemcpy of the backdrop failed")
            self.set_backdrop_device(buf.value)
            self.synchronize()  # (the library's copy is queued: the buffer goes only behind it)
        finally:
            hip.hipFree(buf)

    def _through_device(self, nbytes, fill, out):
        """out (a host array) = what fill(device address) queues into a temporary device buffer of nbytes."""
        hip = self._hip()
        self.synchronize()  # (also makes the context's device this thread's current one: the buffer must live there)
        buf = C.c_void_p()
        if hip.hipMalloc(C.byref(buf), C.c_size_t(max(nbytes, 16))) != 0:
            raise MemoryError("hipMalloc of %d bytes failed" % nbytes)
        try:
            fill(buf.value)
            self.synchronize()
            if hip.hipMemcpy(_p(out), buf, C.c_size_t(nbytes), 2) != 0:  # hipMemcpyDeviceToHost
                raise RuntimeError("hipMemcpy from the device failed")
        finally:
            hip.hipFree(buf)

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
