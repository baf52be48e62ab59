"""GPU tests of the pixel-weight plane (include/splat2d_weights.h).

Yardsticks, none of them the code under test:
  * the context WITHOUT a plane: a plane of ones must give its bytes (gradient image, terms, gradients, trained state), a plane
    that is 4 or 1/4 everywhere exactly that multiple of its gradient image, a binary mask its gradient image where the mask is 1;
  * tests/weights_ref.py: the float64 torch evaluation of L_omega (held to an independent NumPy one by
    tests/test_pixel_weights_cpu.py) and the SAME evaluation in float32 on the same image0; the bar for the gradient image is that
    of tests/test_gpu_loss.py, max |gpu - ref64| <= 4 * max |ref32 - ref64|, for the reason DESIGN.md section 13 gives;
  * the exact sums of the exact products for the totals;
  * the library's own composition: s2d_backward_image_grads fed the gradient image, s2d_step_loss (1, 0, 0) for s2d_step.
Every case prints its figures; DESIGN.md section 26 records them.  Device buffers are torch tensors.
"""
import ctypes as C
import functools
import importlib
import math
import os
import re
import subprocess

import numpy as np
import pytest

import loss_ref as LR
import oracle_lib as O
import weights_ref as WR

pytestmark = pytest.mark.gpu

S2D = importlib.import_module("2dgaussiansplatting_amd")
COARSE = importlib.import_module("2dgaussiansplatting_amd.coarse")
BACKDROP = importlib.import_module("2dgaussiansplatting_amd.backdrop")
MINI = os.path.join(O.GOLDEN, "squirrel_cls_mini_268x213.s2di")
N_MINI = 1024
RANDOM_SCENES = {"7x5": (7, 5, 20, 14), "40x1": (40, 1, 30, 13), "33x17": (33, 17, 200, 11), "96x80": (96, 80, 300, 12)}
SCENES = ["%s-%s" % (s, c) for s in RANDOM_SCENES for c in ("noise", "smooth")]
DSSIM_WEIGHTINGS = [(0.0, 0.0, 1.0), (0.0, 0.8, 0.2), (0.5, 0.3, 0.2)]   # of tests/test_gpu_loss.py: the bar below is theirs
GRAD_FACTOR = 4.0
MSE_W = (1.0, 0.0, 0.0)
INVALID, STATE = 1, 5
MODES = {"plain": {}, "fp16_images": {"fp16_images": True}}


def _torch():
    import torch
    return torch


def random_splats(W, H, n, seed):
    """Explicit random splats, as tests/test_gpu_loss.py draws them."""
    rng = np.random.default_rng(seed)
    s = np.zeros(n, dtype=O.SPLAT_DTYPE)
    s["pos"][:, 0] = rng.uniform(0, W - 1, n)
    s["pos"][:, 1] = rng.uniform(0, H - 1, n)
    s["sx"] = rng.uniform(1.0, 6.0, n)
    s["sy"] = rng.uniform(1.0, 6.0, n)
    s["rot"] = rng.uniform(-np.pi, np.pi, n)
    s["color"] = rng.uniform(0, 1, (n, 3))
    s["opacity"] = rng.uniform(0.1, 1.0, n)
    return s


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> (target, splats).  "<W>x<H>-noise" / "-smooth": random splats on a random-noise or the smooth synthetic target."""
    size, content = name.split("-")
    W, H, n, seed = RANDOM_SCENES[size]
    tgt = LR.noise_image(W, H, 100 + seed) if content == "noise" else O.synthetic_target(W, H)
    return np.ascontiguousarray(tgt, dtype=np.float32), random_splats(W, H, n, seed)


def trainer(name, plane=None, **kw):
    tgt, splats = scene(name)
    t = S2D.WeightedTrainer(tgt.shape[1], tgt.shape[0], len(splats), **kw)
    t.set_target(tgt)
    t.set_splats(splats.view(S2D.SPLAT_DTYPE))
    if plane is not None:
        t.set_pixel_weights(plane)
    return t


def plane_of(name, kind):
    tgt = scene(name)[0]
    return WR.plane(kind, tgt.shape[1], tgt.shape[0], seed=tgt.shape[1])


def device_image(t, fill=float("nan")):
    torch = _torch()
    buf = torch.full((t.H, t.W, 4), fill, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    return buf


def image0_of(t):
    buf = device_image(t)
    t.get_image_rows_device(buf.data_ptr())
    t.synchronize()
    return buf.cpu().numpy()


def loss_grad(t, w):
    buf = device_image(t)
    t.loss_image_grads_device(buf.data_ptr(), *w)
    t.synchronize()
    return buf.cpu().numpy()


def terms_bytes(d):
    return np.array([d[k] for k in ("mse", "l1", "dssim", "total")], dtype=np.float64).tobytes()


def state_bytes(t):
    adams = t.get_adam()
    return t.get_splats().tobytes(), adams[0].tobytes(), adams[1:]


def _fp16(a):
    return a.astype(np.float16).astype(np.float32)


# ---------------------------------------------------------------------------------------------
# 1. a plane of ones is no plane
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name", SCENES)
def test_a_plane_of_ones_gives_the_bytes_of_a_context_without_one(name, mode):
    kw = dict(deterministic=True, **MODES[mode])
    ones = plane_of(name, "ones")
    with trainer(name, **kw) as a, trainer(name, ones, **kw) as b:
        assert a.pixel_weights()[0] is None and b.pixel_weights()[0].tobytes() == ones.tobytes()
        assert b.pixel_weights()[1] == ones.size
        a.forward(); b.forward()
        for w in WR.WEIGHTINGS:
            ga, gb = loss_grad(a, w), loss_grad(b, w)
            assert np.abs(ga[..., :3]).max() > 0 and ga.tobytes() == gb.tobytes(), (name, mode, w)
            assert terms_bytes(a.loss_terms()) == terms_bytes(b.loss_terms())
            a.loss_backward(*w); b.loss_backward(*w)
            assert a.get_grads().tobytes() == b.get_grads().tobytes()
            assert terms_bytes(a.loss_terms()) == terms_bytes(b.loss_terms()) and a.mse() == b.mse()
            wt = b.weighted_terms()                      # under ones the weighted terms are the plain ones
            assert wt["weight_sum"] == ones.size and wt["mse"] == a.loss_terms()["mse"] and wt["total"] == a.loss_terms()["total"]
    for w in WR.WEIGHTINGS:
        with trainer(name, **kw) as a, trainer(name, ones, **kw) as b:
            la, ma = a.step_loss(5, *w)
            lb, mb = b.step_loss(5, *w)
            assert state_bytes(a) == state_bytes(b), (name, mode, w)
            assert la.tobytes() == lb.tobytes() and ma.tobytes() == mb.tobytes()


# ---------------------------------------------------------------------------------------------
# 2. a constant plane scales the gradient image exactly, D-SSIM included
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor", [4.0, 0.25])
@pytest.mark.parametrize("name", SCENES)
def test_a_constant_plane_scales_the_gradient_image_exactly(name, factor):
    const = plane_of(name, "ones") * np.float32(factor)
    with trainer(name) as a, trainer(name, const) as b:
        a.forward(); b.forward()
        for w in WR.WEIGHTINGS + [(0.0, 0.0, 1.0)]:
            ga, gb = loss_grad(a, w), loss_grad(b, w)
            assert np.array_equal(gb, ga * np.float32(factor)), (name, factor, w)   # (a power of two: the product is exact)
            ta, tb = a.loss_terms(), b.loss_terms()
            assert tb["mse"] == ta["mse"] and tb["total"] == pytest.approx(factor * ta["total"], rel=1e-15)


# ---------------------------------------------------------------------------------------------
# 3. a binary mask without the window term
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name", SCENES)
def test_a_binary_mask_keeps_or_zeroes_the_pointwise_gradient(name, mode):
    mask = plane_of(name, "mask")
    with trainer(name, **MODES[mode]) as a, trainer(name, mask, **MODES[mode]) as b:
        a.forward(); b.forward()
        for w in [(1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.5, 0.3, 0.0)]:
            ga, gb = loss_grad(a, w), loss_grad(b, w)
            assert ga[mask == 1].tobytes() == gb[mask == 1].tobytes() and np.abs(ga[mask == 1][:, :3]).max() > 0
            assert (gb[mask == 0] == 0).all() and np.abs(ga[mask == 0][:, :3]).max() > 0, (name, mode, w)


# ---------------------------------------------------------------------------------------------
# 4. a general plane: the gradient image against the float64 reference
# ---------------------------------------------------------------------------------------------
def check_gradient_image(t, tgt, om, label):
    t.forward()
    x = image0_of(t)
    worst = 0.0
    for w in DSSIM_WEIGHTINGS:
        got = loss_grad(t, w)
        assert not got[..., 3].any(), ".w of the gradient image is 0"
        r64, r32 = WR.torch_wloss(x, tgt, om, w), WR.torch_wloss(x, tgt, om, w, "float32")
        e32 = np.abs(r32["grad"] - r64["grad"]).max()
        err = np.abs(got[..., :3].astype(np.float64) - r64["grad"]).max()
        print("%s w=%s: max|grad| %.3g  ref32 error %.3g  gpu error %.3g  ratio %.2f" % (label, w, np.abs(r64["grad"]).max(), e32, err, err / e32))
        worst = max(worst, err / e32)
        assert err <= GRAD_FACTOR * e32, (label, w, err, e32)
        assert loss_grad(t, w).tobytes() == got.tobytes()   # two calls give the same bytes
    return worst


@pytest.mark.parametrize("kind", ["random", "mask"])
@pytest.mark.parametrize("name", SCENES)
def test_gradient_image_matches_the_float64_reference(name, kind):
    om = plane_of(name, kind)
    with trainer(name, om) as t:
        print("%s %s: worst ratio %.2f" % (name, kind, check_gradient_image(t, scene(name)[0], om, "%s %s" % (name, kind))))


@pytest.mark.parametrize("name", ["33x17-noise", "96x80-smooth"])
def test_gradient_image_with_fp16_images(name):
    om = plane_of(name, "random")
    with trainer(name, om, fp16_images=True) as t:
        check_gradient_image(t, _fp16(scene(name)[0]), om, name + " fp16")


# ---------------------------------------------------------------------------------------------
# 5. the totals
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["random", "mask"])
@pytest.mark.parametrize("name", ["7x5-noise", "40x1-smooth", "33x17-noise", "96x80-smooth"])
def test_the_weighted_totals(name, kind):
    tgt = scene(name)[0]
    om = plane_of(name, kind)
    H, W = om.shape
    n, n3 = W * H, 3.0 * W * H
    bound = 2.0 * (n - 1) * 2.0 ** -53   # a double sum of n non-negative addends against their exact sum, any order
    floor = 2.0 ** -23
    with trainer(name, om) as t:
        assert abs(t.pixel_weights()[1] - float(om.astype(np.float64).sum())) <= bound * float(om.astype(np.float64).sum())
        t.forward()
        x = image0_of(t)
        s_om, s_wsq, s_wl1 = WR.weighted_sums_exact(x, tgt, om)
        want_mse = LR.sqerr255_exact(x, tgt) / 255.0 ** 2 / n3
        for w in WR.WEIGHTINGS + [(0.0, 0.0, 1.0), (0.0, 1.0, 0.0)]:
            t.loss_backward(*w)
            got, plain = t.weighted_terms(), t.loss_terms()
            r64, r32 = WR.torch_wloss(x, tgt, om, w), WR.torch_wloss(x, tgt, om, w, "float32")
            assert abs(got["weight_sum"] - s_om) <= bound * s_om
            assert abs(got["mse"] - s_wsq / 255.0 ** 2 / n3) <= bound * got["mse"], (got["mse"], s_wsq / 255.0 ** 2 / n3)
            # mse of s2d_loss_get and s2d_get_mse: the unweighted squared error, the reference's number
            assert abs(plain["mse"] - want_mse) <= bound * want_mse and plain["mse"] != got["mse"]
            assert abs(t.mse() - plain["mse"] * 255.0 ** 2) <= 1e-15 * t.mse()
            if w[1] > 0:
                assert abs(got["l1"] - s_wl1 / n3) <= bound * got["l1"] and got["l1"] == plain["l1"]
                assert abs(got["l1"] - r64["l1"]) <= floor * r64["l1"]
            else:
                assert math.isnan(got["l1"]) and math.isnan(plain["l1"])
            if w[2] > 0:
                bar = max(GRAD_FACTOR * abs(r32["dssim"] - r64["dssim"]) / r64["dssim"], floor)
                rel = abs(got["dssim"] - r64["dssim"]) / r64["dssim"]
                print("%s %s w=%s: dssim %.9g  ref32 rel. error %.3g  gpu rel. error %.3g" % (name, kind, w, got["dssim"],
                      abs(r32["dssim"] - r64["dssim"]) / r64["dssim"], rel))
                assert rel <= bar and got["dssim"] == plain["dssim"], (name, w, rel, bar)
            else:
                assert math.isnan(got["dssim"]) and math.isnan(plain["dssim"])
            bar = max(GRAD_FACTOR * abs(r32["total"] - r64["total"]) / r64["total"], floor)
            assert abs(got["total"] - r64["total"]) <= bar * r64["total"] and got["total"] == plain["total"]


# ---------------------------------------------------------------------------------------------
# 6. composition, deterministic
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("density", [False, True], ids=["plain", "density_stats"])
def test_loss_backward_is_the_gradient_image_through_backward_image_grads(density):
    name, w = "96x80-noise", (0.5, 0.3, 0.2)
    om = plane_of(name, "random")
    with trainer(name, om, deterministic=True) as a, trainer(name, om, deterministic=True) as b:
        a.forward(); a.loss_backward(*w, skip_opacity_grad=False, density_stats=density)
        b.forward()
        buf = device_image(b)
        b.loss_image_grads_device(buf.data_ptr(), *w)
        b.backward_image_grads(buf.data_ptr(), skip_opacity_grad=False, density_stats=density)
        assert np.abs(a.get_grads().view(np.float32)).max() > 0
        assert a.get_grads().tobytes() == b.get_grads().tobytes()
        if density:
            (sa, pa), (sb, pb) = a.density(), b.density()
            assert pa == pb == 1 and sa.any() and sa.tobytes() == sb.tobytes()


def test_step_and_forward_backward_follow_the_plane():
    name = "96x80-noise"
    om = plane_of(name, "random")
    make = lambda: trainer(name, om, deterministic=True)
    with make() as a, make() as b, trainer(name, deterministic=True) as plain:
        mse_a = a.step(3)
        loss_b, mse_b = b.step_loss(3, *MSE_W)
        assert state_bytes(a) == state_bytes(b) and mse_a.tobytes() == mse_b.tobytes()
        assert a.weighted_terms()["total"] == loss_b[-1]
        plain.step(3)
        assert state_bytes(plain)[0] != state_bytes(a)[0]        # ... and that is another training than the unweighted one
    with make() as a, make() as b, make() as c:
        a.forward_backward()
        b.forward(); b.backward()
        c.forward(); c.loss_backward(*MSE_W)
        assert np.abs(a.get_grads().view(np.float32)).max() > 0
        assert a.get_grads().tobytes() == b.get_grads().tobytes() == c.get_grads().tobytes()
        assert a.mse() == b.mse() == c.mse()
        assert a.get_image_rows().tobytes() == b.get_image_rows().tobytes()


# ---------------------------------------------------------------------------------------------
# 7. a masked-out region does not train
# ---------------------------------------------------------------------------------------------
def _deep_inside(splats, edge):
    """Splats whose 3 sigma rectangle (at most 3 * max(sx, sy) to every side, whatever the rotation) ends at a pixel that is
    more than 5 columns left of `edge`: no pixel they touch is within the window's reach of a counted one."""
    reach = splats["pos"][:, 0] + 3.0 * np.maximum(splats["sx"], splats["sy"]) + 1.0
    return np.nonzero(reach <= edge - 6)[0]


def test_the_masked_scene_has_enough_splats_deep_inside():
    assert len(_deep_inside(scene("96x80-noise")[1], 48)) >= 10


def test_a_masked_out_region_does_not_train():
    name, w = "96x80-noise", (0.0, 0.8, 0.2)
    om = np.ones((80, 96), dtype=np.float32)
    om[:, :48] = 0.0
    inside = _deep_inside(scene(name)[1], 48)
    assert len(inside) >= 10
    with trainer(name, om) as t:
        t.forward()
        t.loss_backward(*w, skip_opacity_grad=False)
        g = t.get_grads().view(np.float32).reshape(-1, 9)
        assert not g[inside].any() and np.abs(g).max() > 0
        outside = np.setdiff1d(np.arange(t.n), inside)
        assert (np.abs(g[outside]).max(axis=1) > 0).sum() > len(outside) // 2
    with trainer(name, om) as t:
        t.optimize_opacity = True
        before_s, before_a = t.get_splats().copy(), t.get_adam()[0].copy()
        loss, _ = t.step_loss(5, *w)
        after_s, after_a = t.get_splats(), t.get_adam()[0]
        assert np.isfinite(loss).all()
        for i in inside:                                           # 9 parameters and 18 moments, byte for byte
            assert before_s[i].tobytes() == after_s[i].tobytes() and before_a[i].tobytes() == after_a[i].tobytes(), i
        assert before_s.tobytes() != after_s.tobytes()


# ---------------------------------------------------------------------------------------------
# 8. it trains
# ---------------------------------------------------------------------------------------------
def test_training_under_an_emphasis_lowers_the_weighted_loss():
    """Measured on an MI355X: see DESIGN.md section 26 (the case prints the square's plain MSE of both runs; one run each)."""
    w = (0.0, 0.8, 0.2)
    tgt = O.target_rgba32f(O.load_s2di(MINI))
    H, W = tgt.shape[:2]
    om = np.ones((H, W), dtype=np.float32)
    y0, x0 = (H - 96) // 2, (W - 96) // 2
    om[y0:y0 + 96, x0:x0 + 96] = 4.0

    def square_mse(t):
        t.forward()
        d = (t.get_image_rows()[y0:y0 + 96, x0:x0 + 96, :3].astype(np.float64) - tgt[y0:y0 + 96, x0:x0 + 96, :3]) * 255.0
        return float((d * d).mean())
    with S2D.WeightedTrainer(W, H, N_MINI) as a, S2D.WeightedTrainer(W, H, N_MINI) as b:
        for t in (a, b):
            t.set_target(tgt)
            t.init()
        a.set_pixel_weights(om)
        loss, mse = a.step_loss(40, *w)
        assert np.isfinite(loss).all() and np.isfinite(mse).all() and np.isfinite(a.get_splats().view(np.float32)).all()
        assert loss[-1] < loss[0]
        loss_b, _ = b.step_loss(40, *w)
        assert np.isfinite(loss_b).all()
        print("plain MSE of the centred 96 x 96 square after 40 iterations (one run each): with the plane %.2f, without %.2f; "
              "weighted loss %.6f -> %.6f" % (square_mse(a), square_mse(b), loss[0], loss[-1]))


# ---------------------------------------------------------------------------------------------
# 9. statuses
# ---------------------------------------------------------------------------------------------
def _refused(code, f, *args, **kw):
    with pytest.raises(S2D.S2DError) as ei:
        f(*args, **kw)
    assert ei.value.code == code, ei.value
    return str(ei.value)


REMOVE = "s2d_set_pixel_weights(ctx, NULL)"


def test_refusals_leave_a_context_that_trains():
    torch = _torch()
    name = "96x80-noise"
    om = plane_of(name, "random")
    with trainer(name, deterministic=True) as t:
        COARSE.apply_coarse_signatures(t.L)
        BACKDROP.apply_backdrop_signatures(t.L)
        _refused(INVALID, t.weighted_terms)                                        # no plane
        t.set_pixel_weights(om)
        _refused(STATE, t.weighted_terms)                                          # a plane, no loss pass under it
        buf = device_image(t, 0.0)
        # what cannot follow the plane
        assert REMOVE in _refused(INVALID, COARSE.CoarseTrainer.step_view, t, 1, 48, 40, zoom=0.5)
        assert np.isfinite(t.step(1)).all()
        half = torch.zeros((40, 48, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        assert REMOVE in _refused(INVALID, t.view_backward_device, half.data_ptr(), 48, 40, zoom=0.5, from_target=True)
        assert REMOVE in _refused(INVALID, t.view_grads, half.data_ptr(), 48, 40, zoom=0.5, from_target=True)
        assert np.isfinite(t.step(1)).all()
        t.view_backward_device(half.data_ptr(), 48, 40, zoom=0.5)                  # the caller's own upstream gradient: untouched
        t.view_release()
        BACKDROP.BackdropTrainer.set_backdrop(t, [1.0, 1.0, 1.0])
        t.forward()
        assert REMOVE in _refused(INVALID, BACKDROP.BackdropTrainer.backdrop_grads, t, 0, buf.data_ptr())
        out = device_image(t, 0.0)
        BACKDROP.BackdropTrainer.backdrop_grads(t, buf.data_ptr(), out.data_ptr())  # with an upstream: the caller's loss
        BACKDROP.BackdropTrainer.set_backdrop(t, None)
        assert np.isfinite(t.step(1)).all()
        # planes that are none: the old one survives each
        for bad_value, word in ((float("nan"), "NaN"), (float("inf"), "NaN"), (-1e-30, "NaN")):
            bad = om.copy()
            bad[17, 33] = bad_value
            assert word in _refused(INVALID, t.set_pixel_weights, bad)
            assert t.pixel_weights()[0].tobytes() == om.tobytes()
            assert np.isfinite(t.step(1)).all()
        assert "zero" in _refused(INVALID, t.set_pixel_weights, np.zeros_like(om))
        dev = torch.full((80, 96), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        _refused(INVALID, t.set_pixel_weights_device, dev.data_ptr())
        _refused(INVALID, t.set_pixel_weights_device, dev.data_ptr() + 4)
        plane, total = t.pixel_weights()
        assert plane.tobytes() == om.tobytes() and total == pytest.approx(float(om.astype(np.float64).sum()), rel=1e-12)
        assert np.isfinite(t.step(1)).all()
        # the device setter takes what the host setter takes
        dev = torch.from_numpy(om * np.float32(0.5)).cuda()
        torch.cuda.synchronize()
        t.set_pixel_weights_device(dev.data_ptr())
        assert t.pixel_weights()[0].tobytes() == (om * np.float32(0.5)).tobytes()
        _refused(STATE, t.loss_terms)                                              # a new plane forgets the last terms
        t.set_pixel_weights(om)
        # a held set (s2d_halo_commit) under a plane: the passes and the setters refuse; holding every splat again: accepted
        masks = torch.ones(t.n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        t.halo_commit(masks.data_ptr(), 0)
        assert REMOVE in _refused(INVALID, t.step, 1)
        _refused(INVALID, t.set_pixel_weights, om)
        t.halo_commit(0, 0)
        assert np.isfinite(t.step(1)).all()
    for kw in ({"row_begin": 16, "row_end": 48}, {"count_pairs": True}, {"coverage": True}):
        with trainer(name, **kw) as t:
            _refused(INVALID, t.set_pixel_weights, om)
            assert t.pixel_weights() == (None, 0.0)
            assert np.isfinite(t.step(1)).all()


def test_removing_the_plane_restores_the_plain_step():
    name = "96x80-noise"
    om = plane_of(name, "random")
    with trainer(name, deterministic=True) as a, trainer(name, deterministic=True) as b:
        b.set_pixel_weights(om)
        b.forward()
        weighted = loss_grad(b, MSE_W)                   # (touches neither the gradients nor the squared-error ring)
        b.set_pixel_weights(None)
        assert b.pixel_weights() == (None, 0.0)
        _refused(STATE, b.loss_terms)                    # the terms of the weighted pass are forgotten
        assert loss_grad(b, MSE_W).tobytes() != weighted.tobytes()
        ma, mb = a.step(3), b.step(3)                    # the fused launch again
        assert state_bytes(a)[:2] == state_bytes(b)[:2] and ma.tobytes() == mb.tobytes()


# ---------------------------------------------------------------------------------------------
# 10. the host tool
# ---------------------------------------------------------------------------------------------
def _write_ppm(path, gray):
    H, W = gray.shape
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (W, H) + np.repeat(gray.astype(np.uint8)[..., None], 3, axis=2).tobytes())


def test_host_tool_weight_image(tmp_path):
    exe = S2D._build.build_host_program()
    base = [exe, "--image", MINI, "--splats", "1024", "--iters", "20", "--deterministic"]
    H, W = 213, 268
    black, mask = str(tmp_path / "black.ppm"), str(tmp_path / "mask.ppm")
    _write_ppm(black, np.zeros((H, W)))
    m = np.zeros((H, W))
    m[:, W // 2:] = 255
    _write_ppm(mask, m)
    plain = subprocess.run(base, capture_output=True, text=True, check=True).stdout.strip().splitlines()
    assert len(plain) == 20 and all(re.fullmatch(r"\d+ itr, mse \d+\.\d{4}", l) for l in plain)
    # omega = 1 + 1 * 0: a plane of ones trains as no plane does; the separate launches add the same squared errors in another
    # order (2 (n - 1) 2^-53 relative), which four printed decimals do not show
    r = subprocess.run(base + ["--weight-image", black, "--weight-gain", "1"], capture_output=True, text=True, check=True)
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 20
    got = [re.fullmatch(r"(\d+) itr, mse (\d+\.\d{4}), wloss (\d+\.\d{6})", l) for l in lines]
    assert all(got), lines
    np.testing.assert_allclose([float(g.group(2)) for g in got], [float(l.split("mse")[1]) for l in plain], rtol=1e-9)
    # a real mask: 20 finite lines
    r = subprocess.run(base + ["--weight-image", mask], capture_output=True, text=True, check=True)
    lines = r.stdout.strip().splitlines()
    got = [re.fullmatch(r"(\d+) itr, mse (\d+\.\d{4}), wloss (\d+\.\d{6})", l) for l in lines]
    assert len(lines) == 20 and all(got), lines
    assert all(math.isfinite(float(g.group(2))) and math.isfinite(float(g.group(3))) for g in got)
    assert float(got[-1].group(3)) < float(got[0].group(3))
