"""Builds (when stale) and loads tests/hostcheck/libs2d_view_check.so: csrc/s2d_view_math.h compiled for the host."""
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
    so = os.path.join(HC_DIR, "libs2d_view_check.so")
    csrc = os.path.join(O.ROOT, "2dgaussiansplatting_amd", "csrc")
    srcs = [os.path.join(HC_DIR, "s2d_view_check.cpp"), os.path.join(csrc, "s2d_view_math.h"), os.path.join(csrc, "s2d_math.h"),
            os.path.join(O.ROOT, "include", "splat2d.h")]
    if not os.path.exists(so) or any(os.path.getmtime(so) < os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-std=c++17", "-o", so, srcs[0], "-lm"])
    L = C.CDLL(so)
    L.vc_config_size.restype = C.c_uint
    L.vc_refused.argtypes = [C.c_void_p]
    L.vc_rows.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, C.c_void_p]
    L.vc_rows.restype = None
    L.vc_resolve2.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.vc_resolve2.restype = None
    L.vc_quantise.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    L.vc_quantise.restype = None
    _lib = L
    return L
