"""Builds (when stale) and loads tests/hostcheck/libs2d_hostcheck.so: csrc/s2d_math.h and host/overlay.h compiled for the
host.  One recipe for every test file that uses it, so that no two of them rebuild the library under each other."""
import ctypes as C
import os
import subprocess

import oracle_lib as O

HC_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostcheck")


def load():
    so = os.path.join(HC_DIR, "libs2d_hostcheck.so")
    srcs = [os.path.join(HC_DIR, "s2d_hostcheck.cpp"),
            os.path.join(O.ROOT, "2dgaussiansplatting_amd", "csrc", "s2d_math.h"),
            os.path.join(O.ROOT, "2dgaussiansplatting_amd", "host", "overlay.h")]
    if not os.path.exists(so) or any(os.path.getmtime(so) < os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-std=c++17", "-I", os.path.join(O.ROOT, "include"),
                               "-o", so, srcs[0], "-lm", "-lz"])
    L = C.CDLL(so)
    L.hc_adam.restype = C.c_float
    L.hc_adam.argtypes = [C.c_void_p, C.c_void_p] + [C.c_float] * 5
    L.hc_adam_n.restype = None
    L.hc_adam_n.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int] + [C.c_float] * 3 + [C.c_int]
    return L
