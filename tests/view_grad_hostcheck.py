"""Builds (when stale) and loads tests/hostcheck/libs2d_view_grad_check.so: view_row_adjoint of csrc/s2d_view_math.h compiled
for the host."""
import ctypes as C
import os
import subprocess

import oracle_lib as O

HC_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostcheck")
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    so = os.path.join(HC_DIR, "libs2d_view_grad_check.so")
    csrc = os.path.join(O.ROOT, "2dgaussiansplatting_amd", "csrc")
    srcs = [os.path.join(HC_DIR, "s2d_view_grad_check.cpp"), os.path.join(csrc, "s2d_view_math.h"), os.path.join(csrc, "s2d_math.h")]
    if not os.path.exists(so) or any(os.path.getmtime(so) < os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-std=c++17", "-o", so, srcs[0], "-lm"])
    L = C.CDLL(so)
    L.vgc_adjoint.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, C.c_void_p]
    L.vgc_adjoint.restype = None
    _lib = L
    return L
