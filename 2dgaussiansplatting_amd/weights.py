"""WeightedTrainer: a per-pixel weight plane for the losses and the step (include/splat2d_weights.h) on top of Trainer -- a mask
that keeps a region from attracting splats, or an emphasis that makes one matter more.

The four entry points are declared in a header of their own, so their signatures stand here, in a table of this module's, and
are applied to the library a trainer was created with.  No torch: device buffers cross as addresses."""
import ctypes as C

import numpy as np

from ._abi import S2D_E_INVALID
from ._handle import S2DError, _p
from .trainer import Trainer, _dev

_vp, _int = C.c_void_p, C.c_int


class _WeightedTerms(C.Structure):
    """s2d_weighted_terms."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("weight_sum", C.c_double), ("mse", C.c_double),
                ("l1", C.c_double), ("dssim", C.c_double), ("total", C.c_double)]


# name -> (argtypes, restype) of the symbols include/splat2d_weights.h declares, in its order
WEIGHTS_SIGNATURES = {
    "s2d_set_pixel_weights": ([_vp, _vp], _int),
    "s2d_set_pixel_weights_device": ([_vp, _vp], _int),
    "s2d_get_pixel_weights": ([_vp, _vp, _vp, _vp], _int),
    "s2d_weighted_loss_get": ([_vp, C.POINTER(_WeightedTerms)], _int),
}
WEIGHTS_SYMBOLS = list(WEIGHTS_SIGNATURES)


def apply_weights_signatures(L):
    """Sets argtypes and restype of the four symbols on the loaded library L; a library without them raises AttributeError."""
    for name, (argtypes, restype) in WEIGHTS_SIGNATURES.items():
        f = getattr(L, name)
        f.argtypes, f.restype = argtypes, restype


class WeightedTrainer(Trainer):
    """A Trainer whose losses weigh every pixel by a plane.  Everything else is Trainer's: while a plane is set, step(),
    backward(), forward_backward(), loss_backward() and step_loss() train on the weighted loss; mse() stays the plain one."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        apply_weights_signatures(self.L)

    @staticmethod
    def of(trainer):
        """`trainer` (a Trainer of one context) as a WeightedTrainer of the same context; the multi-device handle has no plane."""
        if not isinstance(trainer, Trainer):
            raise S2DError(S2D_E_INVALID, "WeightedTrainer.of: a Trainer is needed (the multi-device handle has no pixel weights)")
        apply_weights_signatures(trainer.L)
        trainer.__class__ = WeightedTrainer
        return trainer

    def set_pixel_weights(self, plane):
        """The plane from an (H, W) array of finite values >= 0, not all zero; None removes it (s2d_set_pixel_weights)."""
        if plane is None:
            self._ck(self.L.s2d_set_pixel_weights(self._h, None))
            return
        a = np.ascontiguousarray(plane, dtype=np.float32)
        if a.shape != (self.H, self.W):
            raise S2DError(S2D_E_INVALID, "set_pixel_weights: an (H, W) = (%d, %d) array, or None" % (self.H, self.W))
        self._ck(self.L.s2d_set_pixel_weights(self._h, _p(a)))

    def set_pixel_weights_device(self, ptr):
        """The plane from device memory at `ptr` (H x W float32, 16-byte aligned); 0 or None removes it
        (s2d_set_pixel_weights_device).  The buffer may be reused when the call returns."""
        self._ck(self.L.s2d_set_pixel_weights_device(self._h, _dev(ptr)))

    def pixel_weights(self, want_plane=True):
        """-> (plane, weight_sum): the plane as an (H, W) float32 array (None without one, or with want_plane=False) and the
        sum of its values (0.0 without one)."""
        is_set, total = C.c_int32(), C.c_double()
        self._ck(self.L.s2d_get_pixel_weights(self._h, C.byref(is_set), C.byref(total), None))
        if not is_set.value or not want_plane:
            return None, total.value
        a = np.zeros((self.H, self.W), dtype=np.float32)
        self._ck(self.L.s2d_get_pixel_weights(self._h, C.byref(is_set), C.byref(total), _p(a)))
        return a, total.value

    def weighted_terms(self):
        """-> dict(weight_sum, mse, l1, dssim, total) of the last loss pass under the plane: the weighted sums over 3 * H * W,
        NaN for a term whose weight was 0 (s2d_weighted_loss_get)."""
        t = _WeightedTerms()
        t.struct_size = C.sizeof(_WeightedTerms)
        self._ck(self.L.s2d_weighted_loss_get(self._h, C.byref(t)))
        return {"weight_sum": t.weight_sum, "mse": t.mse, "l1": t.l1, "dssim": t.dssim, "total": t.total}
