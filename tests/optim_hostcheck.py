"""Builds (when stale) and loads tests/hostcheck/libs2d_optim_check.so: csrc/s2d_optim_rates.h compiled for the host."""
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
    so = os.path.join(HC_DIR, "libs2d_optim_check.so")
    srcs = [os.path.join(HC_DIR, "s2d_optim_check.cpp"),
            os.path.join(O.ROOT, "2dgaussiansplatting_amd", "csrc", "s2d_optim_rates.h"),
            os.path.join(O.ROOT, "include", "splat2d.h")]
    if not os.path.exists(so) or any(os.path.getmtime(so) < os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-std=c++17", "-o", so, srcs[0], "-lm"])
    L = C.CDLL(so)
    L.oc_config_size.restype = C.c_uint
    L.oc_refused.argtypes = [C.c_void_p]
    L.oc_rates_at.argtypes = [C.c_void_p, C.c_float, C.c_int32, C.c_void_p]
    L.oc_rates_at.restype = None
    L.oc_group_of.argtypes = [C.c_int]
    _lib = L
    return L
