"""A handle of the library: what Trainer (s2d_ctx, `s2d_*`) and MultiTrainer (s2d_multi, `s2d_multi_*`) have in common.

Both C handles are created by `<prefix>create`, freed by `<prefix>destroy`, explain a status with `<prefix>last_error` and
carry the same nine state calls under their prefix.  The base resolves those functions once per object, from the library
the object was created with, so a call costs no string lookup and tools may swap the process-wide library between objects.
"""
import ctypes as C

import numpy as np

from ._abi import ADAM_DTYPE, SPLAT_DTYPE, STATUS_NAMES
from ._runtime import load_library


class S2DError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s: %s" % (STATUS_NAMES.get(code, code), msg))
        self.code = code


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class _Handle:
    """Lifetime, status check and the shared state methods; a subclass names its prefix and sets W, H and n before _create."""

    _PREFIX = None
    _SHARED = ("destroy", "last_error", "set_target", "set_target_synthetic", "init_splats", "set_splats", "get_splats",
               "set_adam", "get_adam", "forward", "get_image")
    _ADAM_SHAPE_ASSERTED = True

    def _create(self, *args):
        """self._h = the handle `<prefix>create(*args, &handle)` makes; a refusal raises with the library's message and
        leaves nothing open."""
        self.L = load_library()
        for name in self._SHARED:
            setattr(self, "_" + name, getattr(self.L, self._PREFIX + name))
        h = C.c_void_p()
        rc = getattr(self.L, self._PREFIX + "create")(*args, C.byref(h))
        self._h = h
        if rc != 0:
            msg = self._last_error(h).decode() if h else "%screate rejected the configuration" % self._PREFIX
            if h:
                self._destroy(h)
            self._h = None
            raise S2DError(rc, msg)

    # -- lifetime
    def close(self):
        if getattr(self, "_h", None):
            self._destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _ck(self, rc):
        if rc != 0:
            raise S2DError(rc, self._last_error(self._h).decode())

    # -- state
    def set_target(self, rgba32f):
        a = np.ascontiguousarray(rgba32f, dtype=np.float32)
        assert a.shape == (self.H, self.W, 4), a.shape
        self._ck(self._set_target(self._h, _p(a)))

    def set_target_synthetic(self):
        self._ck(self._set_target_synthetic(self._h))

    def init(self):
        """init(), main.cpp:280-305 (also what the Restart button calls, :828-831)."""
        self._ck(self._init_splats(self._h))

    def set_splats(self, splats):
        a = np.ascontiguousarray(splats, dtype=SPLAT_DTYPE)
        assert a.shape == (self.n,)
        self._ck(self._set_splats(self._h, _p(a)))

    def get_splats(self):
        a = np.zeros(self.n, dtype=SPLAT_DTYPE)
        self._ck(self._get_splats(self._h, _p(a)))
        return a

    def set_adam(self, adams, beta1t, beta2t, iterations):
        a = np.ascontiguousarray(adams, dtype=ADAM_DTYPE)
        assert not self._ADAM_SHAPE_ASSERTED or a.shape == (self.n,)
        self._ck(self._set_adam(self._h, _p(a), float(beta1t), float(beta2t), int(iterations)))

    def get_adam(self):
        a = np.zeros(self.n, dtype=ADAM_DTYPE)
        b1, b2, it = C.c_float(), C.c_float(), C.c_int32()
        self._ck(self._get_adam(self._h, _p(a), C.byref(b1), C.byref(b2), C.byref(it)))
        return a, np.float32(b1.value), np.float32(b2.value), it.value

    def forward(self):
        self._ck(self._forward(self._h))

    def get_image(self):
        a = np.zeros((self.H, self.W, 4), dtype=np.float32)
        self._ck(self._get_image(self._h, _p(a)))
        return a
