"""CPU test of the per-pixel terms of the reference-order validation mode (S2D_CFG_REFERENCE_ORDER).

tests/hostcheck/s2d_refterms_check.cpp compiles s2d_math.h's `reference_terms` -- the function the HIP backward kernel of
that mode evaluates per (pair, pixel) -- for the host and replays one pixel's chain (alpha, T, running colour, the nine
addends) through a stack of splats.  On a 1 x 1 image every gradient of the oracle is a sum of at most one term, so its
dSplats ARE the terms: the comparison is on bits.  Not the product path (that needs a GPU: test_gpu_reference_order.py).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O

HERE = os.path.dirname(os.path.abspath(__file__))
HC_DIR = os.path.join(HERE, "hostcheck")
SEEDS = 2400


@pytest.fixture(scope="module")
def rt():
    so = os.path.join(HC_DIR, "libs2d_refterms_check.so")
    srcs = [os.path.join(HC_DIR, "s2d_refterms_check.cpp"),
            os.path.join(O.ROOT, "2dgaussiansplatting_amd", "csrc", "s2d_math.h")]
    if not os.path.exists(so) or any(os.path.getmtime(so) < os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-std=c++17", "-o", so, srcs[0], "-lm"])
    L = C.CDLL(so)
    L.rt_backward_1x1.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.rt_backward_1x1.restype = None
    L.rt_expf.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.rt_expf.restype = None
    return L


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def draw(rng, n):
    """Parameters as random_splats of tests/oracle_lib.py draws them; the positions lie around the one pixel instead
    of inside a 1 x 1 image (which would put every splat at the origin)."""
    s = np.zeros(n, dtype=O.SPLAT_DTYPE)
    s["pos"] = rng.uniform(-3.0, 4.0, (n, 2))
    s["sx"] = rng.choice([1.0, 1.5, 3.0, 8.0, 40.0, 300.0, 1024.0], n, p=[.15, .15, .3, .3, .06, .03, .01])
    s["sy"] = rng.choice([1.0, 2.0, 6.0, 25.0, 1024.0], n, p=[.2, .3, .4, .09, .01])
    s["rot"] = rng.uniform(-7, 7, n)
    s["color"] = rng.uniform(0, 1, (n, 3))
    s["opacity"] = rng.uniform(0.1, 1.0, n)
    return s


def covers(L, s):
    """Does the reference's loop visit pixel (0, 0) of a 1 x 1 image for this splat (main.cpp:492-514)?"""
    cnt = O.Counters()
    img = np.zeros((1, 1, 4), dtype=np.float32)
    L.s2do_forward_rows(p(s), 1, 1, 1, 0, 1, p(img), C.byref(cnt))
    return cnt.visited == 1


def stack(L, rng, depth):
    out = []
    while len(out) < depth:
        s = draw(rng, 1)
        if covers(L, s):
            out.append(s)
    return np.concatenate(out)


def test_expf_ref_is_the_oracles_libm_expf(rt):
    """s2d_math.h expf_ref against the expf the oracle calls with the switch of main.cpp:51 on, on bits: the arguments of the
    blend (-d2 / 2 <= 0, down to where the result underflows), and the special cases."""
    rng = np.random.default_rng(11)
    xs = np.concatenate([-rng.uniform(0, 12, 200_000), -rng.uniform(0, 110, 50_000), -np.exp(rng.uniform(-40, 0, 50_000)),
                         rng.uniform(0, 90, 20_000), [0.0, -0.0, -87.9, -88.0, -103.9, -104.0, -200.0, 88.7, 88.8, -np.inf,
                                                      np.inf, np.nan]]).astype(np.float32)
    got = np.empty_like(xs)
    rt.rt_expf(p(xs), len(xs), p(got))
    L = O.lib()
    L.s2do_set_exact_exp(1)
    try:
        want = np.array([L.s2do_exp_approx(float(x)) for x in xs], dtype=np.float32)
    finally:
        L.s2do_set_exact_exp(0)
    same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    assert same.all(), xs[~same][:8]


def test_terms_equal_the_oracles_gradients_on_one_pixel(rt):
    L = O.lib()
    total = reached = nonzero = 0
    try:
        for seed in range(SEEDS):
            rng = np.random.default_rng(seed)
            exact = seed % 4 == 3
            L.s2do_set_exact_exp(1 if exact else 0)
            n = 1 + seed % 8
            splats = stack(L, rng, n)
            ref = np.zeros((1, 1, 4), dtype=np.float32)
            ref[0, 0, :3] = rng.uniform(0, 1, 3)
            ref[0, 0, 3] = 1.0
            o = O.OracleTrainer(ref, n)
            o.splats[:] = splats
            o.forward()
            want = o.backward().view(np.float32).reshape(n, 9).copy()
            assert np.isfinite(want).all()
            got = np.zeros((n, 9), dtype=np.float32)
            fin = np.ascontiguousarray(o.image0[0, 0, :3])
            rt.rt_backward_1x1(p(np.ascontiguousarray(splats)), n, p(fin), p(np.ascontiguousarray(ref[0, 0, :3])), int(exact), p(got))
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (seed, exact, got, want)
            total += n
            reached += int(np.any(want != 0, axis=1).sum())
            nonzero += int((want != 0).sum())
    finally:
        L.s2do_set_exact_exp(0)
    # the comparison is not one of zeros: most splats of a stack are reached before the pixel saturates
    assert reached >= total // 2 and nonzero >= 4 * reached, (total, reached, nonzero)
