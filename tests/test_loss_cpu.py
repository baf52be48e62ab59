"""CPU tests of the image losses' yardstick (tests/loss_ref.py) and of the boundary the feature adds.

The two formulations -- torch conv2d + autograd, and NumPy windowed sums with the hand-derived adjoint -- share only the
definition in include/splat2d.h; held together to 1e-12 of the largest gradient magnitude they pin the SSIM gradient the
GPU tests (tests/test_gpu_loss.py) compare the kernels with.
"""
import ctypes as C
import importlib
import os
import subprocess
import tempfile

import numpy as np
import pytest

import loss_ref as LR
import oracle_lib as O

S2D = importlib.import_module("2dgaussiansplatting_amd")

SHAPES = [(7, 5), (40, 1), (33, 17), (96, 80)]  # W x H
WEIGHTS = [(0.0, 0.0, 1.0), (0.0, 0.8, 0.2), (0.5, 0.3, 0.2), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)]


def pair(W, H, content):
    if content == "noise":
        return LR.noise_image(W, H, 1000 + W), LR.noise_image(W, H, 2000 + H)
    return LR.smooth_image(W, H, 0.0), LR.smooth_image(W, H, 0.4)


@pytest.mark.parametrize("content", ["noise", "smooth"])
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_the_two_formulations_agree(shape, content):
    pytest.importorskip("torch")
    x, y = pair(*shape, content)
    for w in WEIGHTS:
        a, b = LR.torch_loss(x, y, w), LR.numpy_loss(x, y, w)
        scale = np.abs(a["grad"]).max()
        assert scale > 0
        assert np.abs(a["grad"] - b["grad"]).max() <= 1e-12 * scale, (w, np.abs(a["grad"] - b["grad"]).max(), scale)
        for k in ("mse", "l1", "dssim", "total"):
            assert (a[k] is None) == (b[k] is None), (w, k)
            if a[k] is not None:
                assert abs(a[k] - b[k]) <= 1e-12 * max(abs(a[k]), 1e-3), (w, k, a[k], b[k])
        assert (a["l1"] is None) == (w[1] == 0) and (a["dssim"] is None) == (w[2] == 0) and a["mse"] is not None


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_equal_images_have_ssim_one_and_no_gradient(shape):
    pytest.importorskip("torch")
    x = LR.noise_image(*shape, 7)
    for f in (LR.torch_loss, LR.numpy_loss):
        r = f(x, x.copy(), (0.0, 0.0, 1.0))
        assert np.abs(r["s"] - 1.0).max() <= 4e-16
        assert abs(r["dssim"]) <= 4e-16
        assert np.abs(r["grad"]).max() <= 1e-12
    # the window is not renormalised at the border: the means there are smaller than inside, and s is 1 all the same
    assert LR.wsum(np.ones((shape[1], shape[0], 1)))[0, 0, 0] < 0.5


def test_sign_of_zero_is_zero():
    pytest.importorskip("torch")
    x, y = pair(33, 17, "noise")
    y[3:9, 4:20] = x[3:9, 4:20]
    for f in (LR.torch_loss, LR.numpy_loss):
        g = f(x, y, (0.0, 1.0, 0.0))["grad"]
        assert not g[3:9, 4:20].any()
        assert set(np.unique(g)) == {-1.0, 0.0, 1.0}


def test_mse_weights_give_the_reference_gradient_bytes():
    """Weights (1, 0, 0): dL/dx = x - y, the subtraction of main.cpp:616 -- in fp32 a lone subtraction has one result."""
    pytest.importorskip("torch")
    x, y = pair(96, 80, "noise")
    want = (x[..., :3] - y[..., :3]).astype(np.float32)
    assert LR.torch_loss(x, y, (1.0, 0.0, 0.0), "float32")["grad"].astype(np.float32).tobytes() == want.tobytes()
    assert LR.numpy_loss(x, y, (1.0, 0.0, 0.0))["grad"].astype(np.float32).tobytes() == want.tobytes()
    # and the squared error of main.cpp:796-805 on its 255 scale is 255^2 * 3HW * mse up to the fp32 rounding of its terms
    r = LR.numpy_loss(x, y, (1.0, 0.0, 0.0))
    assert abs(LR.sqerr255_exact(x, y) / (255.0 ** 2 * want.size) - r["mse"]) <= 2.0 ** -21 * r["mse"]


def test_loss_struct_layouts_match_header():
    code = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "splat2d.h"
    int main(void) {
        printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(s2d_loss_config), offsetof(s2d_loss_config, struct_size),
               offsetof(s2d_loss_config, w_mse), offsetof(s2d_loss_config, w_l1), offsetof(s2d_loss_config, w_dssim),
               sizeof(s2d_loss_terms), offsetof(s2d_loss_terms, mse), offsetof(s2d_loss_terms, l1),
               offsetof(s2d_loss_terms, dssim), offsetof(s2d_loss_terms, total));
        return 0;
    }'''
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write(code)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(O.ROOT, "include"), src, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    cfg, terms = S2D._LossConfig, S2D._LossTerms
    assert got[:5] == [C.sizeof(cfg), cfg.struct_size.offset, cfg.w_mse.offset, cfg.w_l1.offset, cfg.w_dssim.offset]
    assert got[5:] == [C.sizeof(terms), terms.mse.offset, terms.l1.offset, terms.dssim.offset, terms.total.offset]
    assert got[0] == 16 and got[5] == 32


def test_loss_entry_points_reject_a_null_context():
    S2D._build.build_hip_library()
    lib = S2D.load_library()
    cfg = S2D._LossConfig(C.sizeof(S2D._LossConfig), 0.0, 0.8, 0.2)
    terms = S2D._LossTerms()
    buf = (C.c_double * 4)()
    assert lib.s2d_loss_image_grads_device(None, C.byref(cfg), buf) == 1
    assert lib.s2d_loss_backward(None, C.byref(cfg), 0) == 1
    assert lib.s2d_loss_get(None, C.byref(terms)) == 1
    assert lib.s2d_step_loss(None, 1, 0, C.byref(cfg), buf, buf) == 1
