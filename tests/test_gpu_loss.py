"""GPU tests of the image losses formed by the library (s2d_loss_*, include/splat2d.h "image losses").

Yardsticks, none of them the code under test:
  * tests/loss_ref.py: the float64 torch-CPU evaluation of the definition (held to an independent NumPy one by
    tests/test_loss_cpu.py), and the SAME evaluation in float32 on the same inputs.  The SSIM expression cancels
    (var = E[x^2] - mu^2), so what fp32 loses depends on the image; the bar for the gradient image is
        max |gpu - ref64| <= 4 * max |ref32 - ref64|,
    the factor covering the different rounding of separable sums against 121-tap sums;
  * s2d_backward / s2d_step themselves: with weights (1, 0, 0) the loss is the reference's, and in deterministic mode every
    byte of the gradients, the parameters, the moments must be the existing passes';
  * s2d_backward_image_grads for the density statistics.
Device buffers are torch tensors; a plain Trainer works on its own stream, so both sides synchronise between their work.

Measured on an MI355X (ratio = max |gpu - ref64| / max |ref32 - ref64|, worst of the three weightings): see DESIGN.md
section 13; every case prints its own figures.
"""
import ctypes as C
import functools
import importlib
import math
import os
import subprocess

import numpy as np
import pytest

import loss_ref as LR
import oracle_lib as O

pytestmark = pytest.mark.gpu

S2D = importlib.import_module("2dgaussiansplatting_amd")
MINI = os.path.join(O.GOLDEN, "squirrel_cls_mini_268x213.s2di")
N_MINI = 1024
RANDOM_SCENES = {"7x5": (7, 5, 20, 14), "40x1": (40, 1, 30, 13), "33x17": (33, 17, 200, 11), "96x80": (96, 80, 300, 12)}
WEIGHTS = [(0.0, 0.0, 1.0), (0.0, 0.8, 0.2), (0.5, 0.3, 0.2)]
GRAD_FACTOR = 4.0
INVALID, STATE = 1, 5


def _torch():
    import torch
    return torch


def _fp16(a):
    return a.astype(np.float16).astype(np.float32)


def random_splats(W, H, n, seed):
    """Explicit random splats, as tests/test_gpu_density.py draws them."""
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
def mini_state():
    """The squirrel mini with 1024 splats after 3 oracle steps: target, splats, Adam state."""
    tgt = O.target_rgba32f(O.load_s2di(MINI))
    o = O.OracleTrainer(tgt, N_MINI)
    for _ in range(3):
        o.step()
    return tgt, o.splats.copy(), o.adams.copy(), float(o.beta1t[0]), float(o.beta2t[0]), o.iterations


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> (target, splats).  "<W>x<H>-noise" / "-smooth": random splats on a random-noise or the smooth synthetic target."""
    if name == "mini":
        return mini_state()[:2]
    size, content = name.split("-")
    W, H, n, seed = RANDOM_SCENES[size]
    tgt = LR.noise_image(W, H, 100 + seed) if content == "noise" else O.synthetic_target(W, H)
    return np.ascontiguousarray(tgt, dtype=np.float32), random_splats(W, H, n, seed)


SCENES = ["%s-%s" % (s, c) for s in RANDOM_SCENES for c in ("noise", "smooth")] + ["mini"]


def trainer(name, **kw):
    tgt, splats = scene(name)
    t = S2D.Trainer(tgt.shape[1], tgt.shape[0], len(splats), **kw)
    t.set_target(tgt)
    t.set_splats(splats.view(S2D.SPLAT_DTYPE))
    return t


def mini_trainer(**kw):
    tgt, splats, adams, b1, b2, it = mini_state()
    t = S2D.Trainer(tgt.shape[1], tgt.shape[0], N_MINI, **kw)
    t.set_target(tgt)
    t.set_splats(splats.view(S2D.SPLAT_DTYPE))
    t.set_adam(adams.view(S2D.ADAM_DTYPE), b1, b2, it)
    return t


def device_image(t, fill=float("nan")):
    torch = _torch()
    buf = torch.full((t.H, t.W, 4), fill, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    return buf


def image0_of(t):
    """image0 as s2d_get_image_rows_device returns it (the bytes the reference is fed)."""
    buf = device_image(t)
    t.get_image_rows_device(buf.data_ptr())
    t.synchronize()
    return buf.cpu().numpy()


def loss_grad(t, w, buf=None):
    buf = device_image(t) if buf is None else buf
    t.loss_image_grads_device(buf.data_ptr(), *w)
    t.synchronize()
    return buf.cpu().numpy()


def g9(t):
    return t.get_grads().view(np.float32).reshape(-1, 9)


def check_gradient_image(t, tgt, label):
    """forward(), then the three weightings against the float64 reference under the fp32 reference's own error."""
    t.forward()
    x = image0_of(t)
    assert x.tobytes() == t.get_image_rows().tobytes()
    worst = 0.0
    for w in WEIGHTS:
        got = loss_grad(t, w)
        assert not got[..., 3].any(), ".w of the gradient image is 0"
        r64, r32 = LR.torch_loss(x, tgt, w), LR.torch_loss(x, tgt, w, "float32")
        e32 = np.abs(r32["grad"] - r64["grad"]).max()
        err = np.abs(got[..., :3].astype(np.float64) - r64["grad"]).max()
        print("%s w=%s: max|grad| %.3g  ref32 error %.3g  gpu error %.3g  ratio %.2f" % (label, w, np.abs(r64["grad"]).max(), e32, err, err / e32))
        worst = max(worst, err / e32)
        assert err <= GRAD_FACTOR * e32, (label, w, err, e32)
        if w == WEIGHTS[1]:  # two calls give the same bytes
            assert loss_grad(t, w).tobytes() == got.tobytes()
    return worst


# ---------------------------------------------------------------------------------------------
# 1. the gradient image against the float64 reference
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_gradient_image_matches_the_float64_reference(name):
    with trainer(name) as t:
        check_gradient_image(t, scene(name)[0], name)


@pytest.mark.parametrize("name", ["33x17-noise", "96x80-smooth", "mini"])
def test_gradient_image_with_fp16_images(name):
    """The reference on image0 as returned (fp16 values) and the target rounded to fp16: the arithmetic stays fp32."""
    tgt = scene(name)[0]
    with trainer(name, fp16_images=True) as t:
        t.forward()
        x = image0_of(t)
        assert x[..., :3].tobytes() == _fp16(x[..., :3]).tobytes()
        check_gradient_image(t, _fp16(tgt), name + " fp16")


# ---------------------------------------------------------------------------------------------
# 2. weights (1, 0, 0): the reference's loss, bit for bit
# ---------------------------------------------------------------------------------------------
CASES = {"plain": {}, "fp16_images": {"fp16_images": True}, "index_ranges": {"chunk_pairs": 3000}, "generic_binning": {"generic_binning": True}}
MSE_W = (1.0, 0.0, 0.0)


def mse_bound(W, H):
    return 2.0 * (W * H - 1) * 2.0 ** -53  # two double sums of the same non-negative fp32 terms, any two orders


@pytest.mark.parametrize("opacity", [True, False], ids=["opacity", "skip_opacity"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_mse_weights_reproduce_the_reference_loss_bit_for_bit(case, opacity):
    make = lambda: mini_trainer(deterministic=True, **CASES[case])
    with make() as a, make() as b:
        a.forward(); a.backward(skip_opacity_grad=not opacity)
        b.forward(); b.loss_backward(*MSE_W, skip_opacity_grad=not opacity)
        ga, gb = a.get_grads(), b.get_grads()
        assert np.abs(ga.view(np.float32)).max() > 0
        assert ga.tobytes() == gb.tobytes()
        assert opacity or not gb["opacity"].any()
        assert abs(b.mse() - a.mse()) <= mse_bound(a.W, a.H) * a.mse()
        a.optimize_opacity = b.optimize_opacity = opacity
        a.adam_step(); b.adam_step()
        assert a.get_splats().tobytes() == b.get_splats().tobytes()
        assert a.get_adam()[0].tobytes() == b.get_adam()[0].tobytes()
    with make() as a, make() as b:
        a.optimize_opacity = b.optimize_opacity = opacity
        want_mse = []
        for _ in range(5):
            a.forward(); a.backward(skip_opacity_grad=not opacity)
            want_mse.append(a.mse())
            a.adam_step()
        loss, mse = b.step_loss(5, *MSE_W)
        assert a.get_splats().tobytes() == b.get_splats().tobytes()
        assert a.get_adam()[0].tobytes() == b.get_adam()[0].tobytes()
        assert a.get_adam()[1:] == b.get_adam()[1:]
        assert np.all(np.abs(mse - np.array(want_mse)) <= mse_bound(a.W, a.H) * np.array(want_mse)), (mse, want_mse)
        assert np.all(np.abs(loss - 0.5 * mse / 255.0 ** 2) <= 1e-15 * loss)  # total = w_mse * mse / 2 on the images' scale
        if case == "plain":
            with make() as c:
                c.optimize_opacity = opacity
                step_mse = c.step(5)
                assert c.get_splats().tobytes() == b.get_splats().tobytes()
                assert c.get_adam()[0].tobytes() == b.get_adam()[0].tobytes()
                assert np.all(np.abs(mse - step_mse) <= mse_bound(a.W, a.H) * step_mse)
                assert np.array_equal(b.sqerr_trace(b.get_adam()[3] - 5, 5) / (3.0 * a.W * a.H), mse)  # the ring holds them


# ---------------------------------------------------------------------------------------------
# 3. the loss values
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["7x5-noise", "40x1-smooth", "33x17-noise", "96x80-smooth", "mini"])
def test_loss_terms_match_the_float64_reference(name):
    tgt = scene(name)[0]
    n3 = 3.0 * tgt.shape[0] * tgt.shape[1]
    floor = 2.0 ** -23
    with trainer(name) as t:
        t.forward()
        x = image0_of(t)
        want_mse = LR.sqerr255_exact(x, tgt) / 255.0 ** 2 / n3
        for w in WEIGHTS + [(1.0, 0.0, 0.0), (0.0, 1.0, 0.0)]:
            t.loss_backward(*w)
            got = t.loss_terms()
            r64, r32 = LR.torch_loss(x, tgt, w), LR.torch_loss(x, tgt, w, "float32")
            assert abs(got["mse"] - want_mse) <= mse_bound(t.W, t.H) * want_mse, (got["mse"], want_mse)
            assert abs(t.mse() - got["mse"] * 255.0 ** 2) <= 1e-15 * t.mse()  # the ring of s2d_get_mse holds the same sum
            if w[1] > 0:
                assert abs(got["l1"] - r64["l1"]) <= floor * r64["l1"], (got["l1"], r64["l1"])
            else:
                assert math.isnan(got["l1"])
            if w[2] > 0:
                bar = max(GRAD_FACTOR * abs(r32["dssim"] - r64["dssim"]) / r64["dssim"], floor)
                rel = abs(got["dssim"] - r64["dssim"]) / r64["dssim"]
                print("%s w=%s: dssim %.9g  ref32 rel. error %.3g  gpu rel. error %.3g" % (name, w, got["dssim"],
                      abs(r32["dssim"] - r64["dssim"]) / r64["dssim"], rel))
                assert rel <= bar, (name, w, rel, bar)
            else:
                assert math.isnan(got["dssim"])
            bar = max(GRAD_FACTOR * abs(r32["total"] - r64["total"]) / r64["total"], floor)
            assert abs(got["total"] - r64["total"]) <= bar * r64["total"], (name, w, got["total"], r64["total"])
            t.adam_step()      # (zeroes the gradient buffer; the parameters move, so a fresh frame)
            t.forward()
            x = image0_of(t)
            want_mse = LR.sqerr255_exact(x, tgt) / 255.0 ** 2 / n3


def test_step_loss_reports_the_totals_of_its_iterations():
    w = (0.5, 0.3, 0.2)
    with mini_trainer(deterministic=True) as a, mini_trainer(deterministic=True) as b:
        loss, mse = a.step_loss(4, *w)
        for k in range(4):
            b.forward()
            b.loss_backward(*w, skip_opacity_grad=True)
            assert b.loss_terms()["total"] == loss[k]
            assert b.mse() == mse[k]
            b.adam_step()
        assert a.get_splats().tobytes() == b.get_splats().tobytes()
        assert a.loss_terms()["total"] == loss[3]


# ---------------------------------------------------------------------------------------------
# 4. density statistics ride along
# ---------------------------------------------------------------------------------------------
def test_density_statistics_ride_along():
    w = (0.0, 0.8, 0.2)
    with mini_trainer(deterministic=True) as a, mini_trainer(deterministic=True) as b:
        a.forward(); a.loss_backward(*w, skip_opacity_grad=False, density_stats=True)
        b.forward()
        buf = device_image(b)
        b.loss_image_grads_device(buf.data_ptr(), *w)
        b.backward_image_grads(buf.data_ptr(), skip_opacity_grad=False, density_stats=True)
        (sa, pa), (sb, pb) = a.density(), b.density()
        assert pa == pb == 1 and sa.any()
        assert sa.tobytes() == sb.tobytes()
        assert a.get_grads().tobytes() == b.get_grads().tobytes()
    with mini_trainer() as t:
        loss, _ = t.step_loss(3, *w, density_stats=True)
        stats, passes = t.density()
        assert np.isfinite(loss).all() and passes == 3
        moved = t.relocate(8, float(np.median(stats[:, 2].astype(np.float64) / passes)))  # half of the splats count as starved
        assert 0 < moved <= 8 and t.density()[1] == 0
        assert np.isfinite(t.step_loss(2, *w)[0]).all()


# ---------------------------------------------------------------------------------------------
# 5. statuses
# ---------------------------------------------------------------------------------------------
def _refused(code, f, *args, **kw):
    with pytest.raises(S2D.S2DError) as ei:
        f(*args, **kw)
    assert ei.value.code == code, ei.value


def _all_four_refuse(t, code, w, buf):
    _refused(code, t.loss_image_grads_device, buf.data_ptr(), *w)
    _refused(code, t.loss_backward, *w)
    _refused(code, t.step_loss, 1, *w)


def test_refusals_leave_a_context_that_trains():
    torch = _torch()
    ok = (0.0, 0.8, 0.2)
    with trainer("96x80-noise") as t:
        buf = device_image(t)
        _refused(STATE, t.loss_terms)                                   # no loss pass yet
        _refused(STATE, t.loss_backward, *ok)                           # before forward()
        _refused(STATE, t.loss_image_grads_device, buf.data_ptr(), *ok)
        assert np.isfinite(t.step(1)).all()
        t.forward_backward(skip_image=True)                             # image0 is an older frame
        _refused(STATE, t.loss_backward, *ok)
        _refused(STATE, t.loss_image_grads_device, buf.data_ptr(), *ok)
        assert np.isfinite(t.step(1)).all()
        t.forward()
        for bad in ((-1.0, 0.8, 0.2), (0.0, float("nan"), 0.2), (0.0, 0.0, 0.0), (0.0, 0.8, float("inf")), (0.0, -0.0, -1e-30)):
            _all_four_refuse(t, INVALID, bad, buf)
            assert np.isfinite(t.step(1)).all()
            t.forward()
        cfg = S2D._LossConfig(C.sizeof(S2D._LossConfig) - 4, *ok)      # wrong struct_size, NULL config, NULL / misaligned buffer
        assert t.L.s2d_loss_backward(t._h, C.byref(cfg), 0) == INVALID
        assert t.L.s2d_step_loss(t._h, 1, 0, None, None, None) == INVALID
        assert t.L.s2d_loss_image_grads_device(t._h, None, C.c_void_p(buf.data_ptr())) == INVALID
        _refused(INVALID, t.loss_image_grads_device, 0, *ok)
        _refused(INVALID, t.loss_image_grads_device, buf.data_ptr() + 4, *ok)
        assert np.isfinite(t.step(1)).all()
        # a held set (s2d_halo_commit): refused; holding every splat again: accepted
        masks = torch.ones(t.n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        t.halo_commit(masks.data_ptr(), 0)
        t.forward()
        _all_four_refuse(t, INVALID, ok, buf)
        t.halo_commit(0, 0)
        assert np.isfinite(t.step_loss(1, *ok)[0]).all()
        assert np.isfinite(t.step(1)).all()
    for kw in ({"row_begin": 16, "row_end": 48}, {"count_pairs": True}):
        with trainer("96x80-noise", **kw) as t:
            buf = device_image(t)
            t.forward()
            _all_four_refuse(t, INVALID, ok, buf)
            assert np.isfinite(t.step(1)).all()
    with trainer("96x80-noise", exact_exp=True) as t:                   # the density flag where s2d_backward refuses it
        t.forward()
        _refused(INVALID, t.loss_backward, *ok, density_stats=True)
        _refused(INVALID, t.step_loss, 1, *ok, density_stats=True)
        t.loss_backward(*ok)                                            # ... and without it the mode works
        assert np.isfinite(t.loss_terms()["total"])
        t.adam_step()
        assert np.isfinite(t.step(1)).all()


# ---------------------------------------------------------------------------------------------
# 6. it trains
# ---------------------------------------------------------------------------------------------
def test_training_with_l1_and_dssim_lowers_the_loss_and_the_dssim():
    """Measured on an MI355X: see DESIGN.md section 13 (the case prints both values)."""
    w = (0.0, 0.8, 0.2)
    tgt = scene("mini")[0]

    def final_dssim(t):
        t.forward()
        loss_grad(t, w)
        return t.loss_terms()["dssim"]
    with S2D.Trainer(tgt.shape[1], tgt.shape[0], N_MINI) as a, S2D.Trainer(tgt.shape[1], tgt.shape[0], N_MINI) as b:
        for t in (a, b):
            t.set_target(tgt)
            t.init()
        loss, mse = a.step_loss(60, *w)
        assert np.isfinite(loss).all() and np.isfinite(mse).all()
        assert loss[-1] < loss[0]
        b.step(60)
        da, db = final_dssim(a), final_dssim(b)
        print("dssim after 60 iterations: L1 + D-SSIM training %.6f, MSE training %.6f; loss %.6f -> %.6f" % (da, db, loss[0], loss[-1]))
        assert da < db


# ---------------------------------------------------------------------------------------------
# 7. the host tool
# ---------------------------------------------------------------------------------------------
def test_host_tool_loss_weights():
    exe = S2D._build.build_host_program()
    base = [exe, "--image", MINI, "--splats", "1024"]
    r = subprocess.run(base + ["--iters", "40", "--loss-weights", "0,0.8,0.2"], capture_output=True, text=True, check=True)
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 40
    import re
    losses = []
    for k, line in enumerate(lines):
        m = re.fullmatch(r"(\d+) itr, mse (\d+\.\d{4}), loss (\d+\.\d{6})", line)
        assert m and int(m.group(1)) == k, line
        losses.append(float(m.group(3)))
    assert lines[0].startswith("0 itr, mse 5934.9042, loss ")  # the first frame is the reference's, whatever the loss
    assert losses[-1] < losses[0]
    # without the option: the text of test_cpp_host_loop_prints_the_reference_trace (tests/test_gpu_parity.py)
    r = subprocess.run(base + ["--iters", "12"], capture_output=True, text=True, check=True)
    lines = r.stdout.strip().splitlines()
    want = [5934.9042, 4659.3289, 3634.5384, 2840.9659, 2253.0626, 1839.7870, 1567.4046, 1401.9065,
            1311.3069, 1267.7320, 1248.9938, 1244.4892]
    assert lines[0] == "0 itr, mse 5934.9042" and len(lines) == 12
    assert all(re.fullmatch(r"\d+ itr, mse \d+\.\d{4}", l) for l in lines)
    np.testing.assert_allclose([float(l.split("mse")[1]) for l in lines], want, rtol=2e-5)
    # works with --relocate-every; refused with a message on the multi-device handle
    r = subprocess.run(base + ["--iters", "12", "--loss-weights", "0,0.8,0.2", "--relocate-every", "6", "--relocate-window", "3"],
                       capture_output=True, text=True, check=True)
    assert len(r.stdout.strip().splitlines()) == 12 and "relocated" in r.stderr
    r = subprocess.run(base + ["--iters", "2", "--loss-weights", "0,0.8,0.2", "--gpus", "2"], capture_output=True, text=True)
    assert r.returncode != 0 and "--loss-weights" in r.stderr and not r.stdout
