"""GPU tests of coarse-to-fine fitting (include/splat2d_coarse.h): s2d_step_view, s2d_view_target_device,
CoarseTrainer and `splat2d_train --coarse`.

The yardsticks hold none of the new code:
  * a TWIN context that replays the iterations with the calls that existed before -- render_view for the view,
    view_backward_device(from_target=True) for the gradients, adam_step for the step; in deterministic mode its splats, moments,
    beta powers and iteration count are the bytes s2d_step_view must leave;
  * coarse_ref.mse255 of the twin's view and the target, evaluated before each of its steps, for mse_out: any double sum of the
    same fp32 terms lies within 2 (n - 1) 2^-53 of the exact one (loss_ref.sqerr255_exact), the bar is relative 1e-12;
  * s2d_step for the identity view with the context's own target;
  * the NumPy restatement of the resample (coarse_ref.resample), in bytes.
Scenes: those of tests/view_ref.py (64 x 48, n = 600) and the squirrel mini."""
import ctypes as C
import functools
import importlib
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import coarse_ref as R
import oracle_lib as O
import view_ref as V
from view_grad_cases import _torch, dev, g9, scene, vkw

pytestmark = pytest.mark.gpu

S2D = importlib.import_module("2dgaussiansplatting_amd")
W, H, N = V.SRC_W, V.SRC_H, V.N_SPLATS
MINI = os.path.join(O.GOLDEN, "squirrel_cls_mini_268x213.s2di")
E_INVALID, E_NONFINITE, E_NOMEM = 1, 3, 4
F = np.float32
STRIP = ((0.0, 16.0), 128.25, 0.0, (8208, 32))   # 513 x 2 = 1026 tiles: beyond kSqerrSmallTiles = 1024
FAR = ((1000.0, 1000.0), 1.0, 0.0, (40, 24))     # every splat off the window: every tile's list is empty


def context(splats, **kw):
    t = S2D.CoarseTrainer(W, H, len(splats), **kw)
    t.set_target_synthetic()
    t.set_splats(np.ascontiguousarray(splats).view(S2D.SPLAT_DTYPE))
    return t


def state(t):
    ad = t.get_adam()
    return t.get_splats().tobytes(), ad[0].tobytes(), (float(ad[1]), float(ad[2]), ad[3])


def view_target(view, seed):
    _, _, _, (ow, oh) = view
    return np.random.default_rng(100 + seed).uniform(0, 1, (oh, ow, 4)).astype(F)


def prepare(t, dead, controls):
    if dead:
        t.set_alive(np.arange(t.n) % 3 != 0)
    if controls:
        t.set_optim(pos=0.5, scale=0.2, rot=0.1, color=0.05, opacity=0.02)
        t.set_frozen(np.arange(t.n) % 5 == 0)


@functools.lru_cache(maxsize=None)
def pair(name, view, samples, iters=3, opacity=False, dead=False, controls=False, deterministic=True, **kw):
    """One case, run once: s2d_step_view on one context, the replay with the existing calls on its twin.
    -> (state after step_view, mse_out, state of the twin, the yardstick's MSE values)."""
    tgt = view_target(view, samples)
    kw = dict(kw, deterministic=deterministic)
    with context(scene(name), **kw) as t, context(scene(name), **kw) as twin:
        prepare(t, dead, controls)
        prepare(twin, dead, controls)
        tg = dev(tgt)
        got_mse = t.step_view(iters, target_ptr=tg.data_ptr(), optimize_opacity=opacity, **vkw(view, samples))
        got = state(t)
        twin.optimize_opacity = opacity
        want_mse = []
        for _ in range(iters):
            want_mse.append(R.mse255(twin.render_view(**vkw(view, samples)), tgt))
            twin.view_backward_device(tg.data_ptr(), from_target=True, skip_opacity_grad=not opacity, **vkw(view, samples))
            twin.adam_step()
        want = state(twin)
    return got, got_mse, want, np.array(want_mse)


# (a), (c) -------------------------------------------------------------------------------------------------------------------
CASES = {
    "v1_s1": ("M", V.VIEWS[0], 1), "v1_s2": ("M", V.VIEWS[0], 2), "v1_s4": ("M", V.VIEWS[0], 4),
    "v2_s1": ("M", V.VIEWS[1], 1), "v2_s2": ("M", V.VIEWS[1], 2), "v3_s1_filter": ("M", V.VIEWS[2], 1), "v4_s1_border": ("M", V.VIEWS[3], 1),
    "sparse_s1": ("S", V.SPARSE_VIEW, 1), "sparse_s2": ("S", V.SPARSE_VIEW, 2), "sparse_s4": ("S", V.SPARSE_VIEW, 4),
    "exact_exp": ("M", V.VIEWS[0], 2, 3, False, False, False, True, ("exact_exp", True)),
    "dead_rows": ("M", V.VIEWS[2], 2, 3, False, True),
    "optimize_opacity": ("M", V.VIEWS[0], 2, 3, True),
    "generic_binning": ("M", V.VIEWS[0], 2, 3, False, False, False, True, ("generic_binning", True)),
    "rates_and_frozen": ("M", V.VIEWS[0], 1, 3, False, False, True),
    "adversarial_scene": ("A", V.VIEWS[0], 2),
}
MSE_ONLY = {"all_lists_empty": ("M", FAR, 1), "strip_1026_tiles": ("M", STRIP, 1, 2), "v5_two_tiles": ("M", V.VIEWS[4], 1)}


def run(case):
    args = list({**CASES, **MSE_ONLY}[case])
    kw = {}
    if len(args) == 9:
        key, value = args.pop()
        kw[key] = value
    return pair(*args, **kw)


@pytest.mark.parametrize("case", list(CASES))
def test_step_view_leaves_the_bytes_of_the_existing_calls(case):
    got, _, want, _ = run(case)
    assert got[2] == want[2] and got[2][2] == 3                       # beta powers, iteration count
    assert got[0] == want[0]                                           # splats
    assert got[1] == want[1]                                           # moments
    assert got[0] != scene(CASES[case][0]).tobytes()                   # and something was trained


@pytest.mark.parametrize("case", list(CASES) + list(MSE_ONLY))
def test_mse_out_is_the_error_of_the_view_before_each_step(case):
    _, got, _, want = run(case)
    print("\n[step_view mse] %s: %s, worst relative difference %.2e" % (case, got, np.abs(got / want - 1).max()))
    assert np.isfinite(got).all() and (got > 0).all() and len(got) == len(want)
    assert np.abs(got - want).max() <= 1e-12 * want.max() and (np.abs(got - want) <= 1e-12 * want).all()


def test_a_view_without_a_splat_has_the_targets_own_energy():
    _, got, _, _ = run("all_lists_empty")
    tgt = view_target(FAR, 1)
    want = R.mse255(np.zeros_like(tgt), tgt)
    assert (np.abs(got - want) <= 1e-12 * want).all()


def test_two_runs_give_the_same_bytes():
    for case in ("v1_s2", "strip_1026_tiles"):
        first = run(case)
        pair.cache_clear()
        again = run(case)
        assert first[1].tobytes() == again[1].tobytes() and first[0] == again[0], case


# (b) ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,samples", [(0, 2), (1, 1)], ids=["v1_s2", "v2_s1"])
def test_float_atomics_stay_under_the_bars_of_the_training_sweep(k, samples):
    """One iteration on contexts that add with float atomics: the parameters of the two paths agree to the update bar of
    test_training_steps_random_sweep for one step, 1e-3 * 0.05 + 1e-5 * max|parameter|."""
    got, got_mse, want, want_mse = pair("M", V.VIEWS[k], samples, 1, False, False, False, False)
    a = np.frombuffer(got[0], dtype=F).reshape(-1, 9).astype(np.float64)
    b = np.frombuffer(want[0], dtype=F).reshape(-1, 9).astype(np.float64)
    assert got[2] == want[2] and np.abs(a - b).max() <= 1e-3 * 0.05 + 1e-5 * np.abs(b).max(), np.abs(a - b).max()
    assert (np.abs(got_mse - want_mse) <= 1e-12 * want_mse).all()


FIT_VARIANTS = [(exact, samples, need_op, det) for exact in (False, True) for samples in (1, 2, 4) for need_op in (False, True)
                for det in (False, True)]


@pytest.mark.parametrize("exact,samples,need_op,det", FIT_VARIANTS,
                         ids=["%s_s%d_%s_%s" % ("exact" if e else "approx", s, "op" if o else "noop", "det" if d else "atomic")
                              for e, s, o, d in FIT_VARIANTS])
def test_every_view_fit_kernel_variant_against_the_existing_calls(exact, samples, need_op, det):
    """A row for each view_fit_kernel<EXACT, S, NEED_OP, DET>: scene M through view 1 (53 x 37, so raster grids of 53 x 37,
    106 x 74 and 212 x 148: several tiles and partial ones at every S), three iterations.  NEED_OP = false is a step without
    optimize_opacity, on both sides.  Deterministic rows leave the bytes of the twin's view_backward_device(from_target) +
    adam_step.  Rows that add with float atomics are held to the bars of
    test_float_atomics_stay_under_the_bars_of_the_training_sweep; its MSE bar is applied to the first iteration's value, the one
    both contexts form from the same splats -- the later ones are errors of states the order of the atomic additions has already
    let differ, and that bar (the rounding of one double sum) says nothing about them."""
    kw = {"exact_exp": True} if exact else {}
    got, got_mse, want, want_mse = pair("M", V.VIEWS[0], samples, 3, need_op, False, False, det, **kw)
    assert got[2] == want[2] and got[2][2] == 3                       # beta powers, iteration count
    assert got[0] != scene("M").tobytes()                              # something was trained
    assert len(got_mse) == 3 and np.isfinite(got_mse).all() and (got_mse > 0).all()
    if det:
        assert got[0] == want[0]                                       # splats
        assert got[1] == want[1]                                       # moments
        assert (np.abs(got_mse - want_mse) <= 1e-12 * want_mse).all()  # (the bar of test_mse_out_is_the_error_of_the_view_before_each_step)
        return
    a = np.frombuffer(got[0], dtype=F).reshape(-1, 9).astype(np.float64)
    b = np.frombuffer(want[0], dtype=F).reshape(-1, 9).astype(np.float64)
    print("\n[view_fit float atomics] worst parameter difference %.3e (bar %.3e), first mse relative difference %.2e"
          % (np.abs(a - b).max(), 1e-3 * 0.05 + 1e-5 * np.abs(b).max(), abs(got_mse[0] / want_mse[0] - 1)))
    assert np.abs(a - b).max() <= 1e-3 * 0.05 + 1e-5 * np.abs(b).max(), np.abs(a - b).max()
    assert abs(got_mse[0] - want_mse[0]) <= 1e-12 * want_mse[0]


# (d) ------------------------------------------------------------------------------------------------------------------------
def test_identity_view_with_the_contexts_target_is_step():
    tgt = O.synthetic_target(W, H)

    def make():
        t = context(scene("M"), deterministic=True)
        t.set_target(tgt)
        return t

    with make() as a, make() as b:
        first = a.step(2), b.step(2)
        assert first[0].tobytes() == first[1].tobytes()
        before = a.get_image().tobytes(), a.rebuild_count(), a.mse()
        tg = dev(tgt)
        mse_a = a.step_view(3, W, H, target_ptr=tg.data_ptr())
        assert (a.get_image().tobytes(), a.rebuild_count(), a.mse()) == before   # the training state, untouched on the view's side
        mse_b = b.step(3)
        sa, sb = state(a), state(b)
        assert sa[2] == sb[2] and sa[2][2] == 5
        assert sa[0] == sb[0] and sa[1] == sb[1]
        print("\n[identity view] step_view %s, step %s" % (mse_a, mse_b))
        assert (np.abs(mse_a - mse_b) <= 1e-12 * mse_b).all()
        both = a.step(2), b.step(2)                                   # and both train on alike
        assert both[0].tobytes() == both[1].tobytes() and state(a) == state(b)


# (e) ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16_images"])
def test_view_target_is_the_restatement_in_bytes(fp16):
    torch = _torch()
    for k, (iw, ih) in enumerate(R.IMAGES):
        image = R.noise_image(iw, ih, k)
        stored = image.astype(np.float16).astype(F) if fp16 else image
        with S2D.CoarseTrainer(iw, ih, 4, fp16_images=fp16) as t:
            t.set_target(image)
            mine = [case for case in R.CASES if case[:3] == (iw, ih, k)]
            assert len(mine) >= 21
            for case in mine:
                _, _, _, origin, zoom, (ow, oh) = case
                want = R.resample(stored, ow, oh, origin, zoom)
                buf = torch.full((oh, ow, 4), float("nan"), dtype=torch.float32, device="cuda")
                torch.cuda.synchronize()
                t.view_target_device(buf.data_ptr(), ow, oh, origin, zoom)
                t.synchronize()
                got = buf.cpu().numpy()
                assert not np.isnan(got).any(), case                   # every pixel of the buffer was written
                assert got.tobytes() == want.tobytes(), case
            _, _, _, origin, zoom, (ow, oh) = mine[2]                 # ... and the same through the host array
            assert t.view_target(ow, oh, origin, zoom).tobytes() == R.resample(stored, ow, oh, origin, zoom).tobytes()


def test_the_librarys_own_target_and_its_staleness():
    view = V.VIEWS[1]                                                   # the whole source at half size
    origin, zoom, _, (ow, oh) = view
    tgt, other = O.synthetic_target(W, H), R.noise_image(W, H, 9)

    def make():
        t = context(scene("M"), deterministic=True)
        t.set_target(tgt)
        return t

    with make() as a, make() as b:
        small = b.view_target(ow, oh, origin, zoom)
        assert small.tobytes() == R.resample(tgt, ow, oh, origin, zoom).tobytes()
        sd = dev(small)
        mse_a = a.step_view(3, **vkw(view, 2))                          # NULL: the library's own
        mse_b = b.step_view(3, target_ptr=sd.data_ptr(), **vkw(view, 2))
        assert mse_a.tobytes() == mse_b.tobytes() and state(a) == state(b)
        a.set_target(other)                                             # the own target is stale now
        want = R.mse255(b.render_view(**vkw(view, 2)), R.resample(other, ow, oh, origin, zoom))
        got = a.step_view(1, **vkw(view, 2))[0]
        assert abs(got - want) <= 1e-12 * want and abs(got - mse_a[-1]) > 1e-3 * want
        a.view_release()
        b.view_release()
        again = a.step_view(1, **vkw(view, 2))[0]                       # allocated and resampled again
        assert np.isfinite(again) and 0 < again


# (f) ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big_buffer():
    torch = _torch()
    buf = torch.zeros((1 << 16) * 4 + 8, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    return buf


def unchanged(t, before):
    return not g9(t.get_grads()).any() and state(t) == before


def test_refusals_leave_the_context_as_it_was(big_buffer):
    good = V.make_config(S2D._ViewConfig)
    base = big_buffer.data_ptr()
    mse = np.zeros(2)
    out = mse.ctypes.data_as(C.c_void_p)
    for kw in ({"coverage": True}, {"count_pairs": True}, {"reference_order": True}):
        with context(scene("M"), **kw) as t:
            before = state(t)
            assert t.L.s2d_step_view(t._h, C.byref(good), C.c_void_p(base), 2, 0, out) == E_INVALID, kw
            assert t.L.s2d_step_view(t._h, C.byref(good), None, 2, 0, out) == E_INVALID, kw
            assert unchanged(t, before), kw
    with S2D.CoarseTrainer(64, 64, 10, row_begin=16, row_end=48) as slab:
        slab.set_target_synthetic()
        slab.init()
        before = state(slab)
        assert slab.L.s2d_step_view(slab._h, C.byref(good), C.c_void_p(base), 2, 0, out) == E_INVALID
        assert state(slab) == before
    with context(scene("M")) as t:
        L, h = t.L, t._h
        before = state(t)
        rgba8 = V.make_config(S2D._ViewConfig, format=1)
        assert L.s2d_step_view(h, C.byref(rgba8), C.c_void_p(base), 2, 0, out) == E_INVALID
        assert L.s2d_view_target_device(h, C.byref(rgba8), C.c_void_p(base)) == E_INVALID
        assert L.s2d_step_view(h, None, C.c_void_p(base), 2, 0, out) == E_INVALID
        for off in (4, 8):
            assert L.s2d_step_view(h, C.byref(good), C.c_void_p(base + off), 2, 0, out) == E_INVALID, off
            assert L.s2d_view_target_device(h, C.byref(good), C.c_void_p(base + off)) == E_INVALID, off
        assert L.s2d_view_target_device(h, C.byref(good), None) == E_INVALID
        tiny = V.make_config(S2D._ViewConfig, zoom=1.0 / 512)           # below 1/256 no target is resampled ...
        assert L.s2d_view_target_device(h, C.byref(tiny), C.c_void_p(base)) == E_INVALID
        assert L.s2d_step_view(h, C.byref(tiny), None, 2, 0, out) == E_INVALID
        assert b"1/256" in L.s2d_last_error(h)
        edge = V.make_config(S2D._ViewConfig, zoom=1.0 / 256, out_width=2, out_height=2, origin_x=0.0, origin_y=0.0)
        assert L.s2d_view_target_device(h, C.byref(edge), C.c_void_p(base)) == 0   # ... at 1/256 it is
        t.synchronize()
        for flags in (0x2, 0x4, 0x8, 0x10, 0x80000000):
            assert L.s2d_step_view(h, C.byref(good), C.c_void_p(base), 2, flags, out) == E_INVALID, flags
        assert b"flags" in L.s2d_last_error(h)
        assert L.s2d_step_view(h, C.byref(good), C.c_void_p(base), -1, 0, out) == E_INVALID
        assert unchanged(t, before)
        assert L.s2d_step_view(h, C.byref(good), C.c_void_p(base), 0, 0, out) == 0      # no iterations: nothing happens
        assert len(t.step_view(0, 32, 24, zoom=0.5)) == 0
        assert unchanged(t, before) and not mse.any()
        assert L.s2d_step_view(h, C.byref(good), C.c_void_p(base + 16), 1, 0x1, out) == 0
        t.synchronize()
        t.step(2)                                                                       # and the context trains on


def test_pair_budget_refuses_and_the_context_trains_on(big_buffer):
    def make():
        t = S2D.CoarseTrainer(W, H, N, deterministic=True, chunk_pairs=4000)  # view 6 needs more than 216 * 60 pairs
        t.set_target_synthetic()
        t.set_splats(scene("M").view(S2D.SPLAT_DTYPE))
        return t

    with make() as t, make() as twin:
        cfg = V.make_config(S2D._ViewConfig, out_width=160, out_height=96, origin_x=20.0, origin_y=10.0, zoom=16.0)
        before = state(t)
        assert t.L.s2d_step_view(t._h, C.byref(cfg), C.c_void_p(big_buffer.data_ptr()), 2, 0, None) == E_NOMEM
        assert b"pairs" in t.L.s2d_last_error(t._h)
        assert unchanged(t, before)
        a, b = t.step(2), twin.step(2)
        assert a.tobytes() == b.tobytes() and state(t) == state(twin)


def test_a_nonfinite_parameter_ends_the_trace_with_nans(big_buffer):
    view = V.VIEWS[1]
    with context(scene("M")) as t:
        t.step_view(2, **vkw(view))
        ad, b1, b2, it = t.get_adam()
        assert it == 2
        ad["mv"][7, 4, 0] = np.inf                                    # first moment of splat 7's rot: its next update is non-finite
        t.set_adam(ad, b1, b2, it)
        mse = np.zeros(5)
        cfg = V.make_config(S2D._ViewConfig, out_width=32, out_height=24, origin_x=0.0, origin_y=0.0, zoom=0.5)
        assert t.L.s2d_step_view(t._h, C.byref(cfg), None, 5, 0, mse.ctypes.data_as(C.c_void_p)) == E_NONFINITE
        assert t.stats()["first_nonfinite_iteration"] == 2
        assert np.isfinite(mse[0]) and np.isnan(mse[1:]).all()        # iteration 2 printed, 3.. never ran
        failed = t.get_splats()
        assert not np.isfinite(failed["rot"][7])
        with pytest.raises(S2D.S2DError) as ei:
            t.step_view(2, **vkw(view))                               # still stopped ...
        assert ei.value.code == E_NONFINITE
        assert t.get_splats().tobytes() == failed.tobytes()           # ... and nothing moved
        assert t.get_adam()[3] == 3


# (g) ------------------------------------------------------------------------------------------------------------------------
def test_host_tool_coarse_stage_is_the_binding(tmp_path):
    tgt = O.target_rgba32f(O.load_s2di(MINI))
    Ht, Wt = tgt.shape[:2]
    ow, oh = math.ceil(Wt * 0.5), math.ceil(Ht * 0.5)
    train = S2D._build.build_host_program()
    ckpt = str(tmp_path / "coarse.ckpt")
    r = subprocess.run([train, "--image", MINI, "--splats", "1024", "--coarse", "0.5:30", "--iters", "60", "--deterministic",
                        "--save-checkpoint", ckpt], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()

    def full_mse(t):
        t.forward()
        d = (t.get_image()[..., :3].astype(np.float64) - tgt[..., :3]) * 255.0
        return float((d * d).mean())

    with S2D.CoarseTrainer(Wt, Ht, 1024, deterministic=True) as t:
        t.set_target(tgt)
        t.init()
        mse0 = full_mse(t)
        t.init()
        coarse = t.step_view(30, ow, oh, zoom=0.5)
        t.view_release()
        after = state(t)
        mse30 = full_mse(t)
        t.set_splats(np.frombuffer(after[0], dtype=S2D.SPLAT_DTYPE))   # (forward() wrote nothing of the state; the lists start as the tool's)
        ad = np.frombuffer(after[1], dtype=S2D.ADAM_DTYPE)
        t.set_adam(ad, *after[2])
        fine = t.step(30)
        want = ["%d itr, mse %.4f" % (k, v) for k, v in enumerate(list(coarse) + list(fine))]
        splats = t.get_splats().tobytes()
    assert len(lines) == 60 and all(re.fullmatch(r"\d+ itr, mse \d+\.\d{4}", l) for l in lines)
    assert lines == want
    raw = open(ckpt, "rb").read()
    head = struct.calcsize("<4s3I2fi")
    assert raw[:4] == b"S2DC" and struct.unpack_from("<i", raw, head - 4)[0] == 60
    assert raw[head:head + len(splats)] == splats
    # an observation, like test_coarse_to_fine_trains: nothing is claimed about how much a schedule buys
    print("\n[host tool --coarse 0.5:30] full-size MSE: start %.2f, after the half-size stage %.2f; trace: view %.2f -> %.2f, full %.2f -> %.2f"
          % (mse0, mse30, coarse[0], coarse[-1], fine[0], fine[-1]))
    assert mse30 < mse0 and np.isfinite([mse0, mse30, fine[-1]]).all()
    # stages that reach the end of the run: the views are released behind the loop, the checkpoint is written as ever
    r = subprocess.run([train, "--image", MINI, "--splats", "64", "--coarse", "0.25:2,0.5:2", "--iters", "4", "--save-checkpoint", ckpt],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and len(r.stdout.strip().splitlines()) == 4, r.stderr[-2000:]
