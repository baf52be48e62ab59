"""GPU tests of the coverage channel (S2D_CFG_COVERAGE) where the plain families are already held to
the oracle and the coverage family was not: adversarial splats on image sizes down to one pixel, the named geometry edges of
tests/test_gpu_parity.py, a strip wider than 512 tile columns and a view wider than 8192 pixels, training against a loop
computed on the CPU, every combination section 22 claims, and the host program.

The comparison scheme is tests/test_gpu_coverage.py's.  BITS against the white twin (coverage_ref.white_twin: the same splats
coloured (1, 0, 0) in a plain context, whose red channel is the coverage operation for operation): image0.w, a view's .w, and
in deterministic contexts the geometric and opacity columns of the backward walk under (0, 0, 0, u); .rgb and the nine columns
under (r, g, b, 0) against a plain context of the same kind; and, without fp16 images, image0.w against the ORACLE's twin.
Gradients are compared with NaN required at the same places and equal floats everywhere else (same_grads), never with `==`
alone.  Where one more addend or another summation order changes a rounding -- a mixed upstream, float atomics -- the bar is
(a) of oracle_lib.grad_bars: 1e-6 of the summed magnitudes of the terms, which coverage_ref.FourChannelOracle reports for the
two oracle passes the four-channel gradient splits into.  Training is held to that loop ("f32") with the bars of
tests/test_gpu_parity.py::test_training_steps_random_sweep; tests/test_coverage_cpu.py shows the loop's own two summation modes
agree ten times better than those bars.
"""
import ctypes as C
import functools
import importlib
import subprocess

import numpy as np
import pytest

import adam_cases as A
import alive_ref as AR
import coverage_ref as CR
import optim_ref as OR
import oracle_lib as O
import test_gpu_coverage as TC

pytestmark = pytest.mark.gpu

S2D = importlib.import_module("2dgaussiansplatting_amd")
GEOM, COLOUR = CR.GEOM, [5, 6, 7]
F32 = np.float32


def f9(a):
    return np.ascontiguousarray(a).view(F32).reshape(-1, 9)


def context(W, H, s9, tgt, **kw):
    """A Trainer holding the target and the (n, 9) splats (none: nothing is set)."""
    s9 = f9(s9)
    t = S2D.Trainer(W, H, len(s9), **kw)
    t.set_target(np.ascontiguousarray(tgt))
    if len(s9):
        t.set_splats(np.ascontiguousarray(s9).view(S2D.SPLAT_DTYPE).reshape(-1))
    return t


def same_grads(a, b):
    """NaN exactly where the other side has NaN, and equal floats elsewhere (a zero's sign may differ: x + 0 * y)."""
    a, b = np.asarray(a), np.asarray(b)
    an, bn = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and bool((an == bn).all()) and bool(np.all(a[~an] == b[~bn]))


def state(t):
    ad, b1, b2, it = t.get_adam()
    return f9(t.get_splats()).copy(), np.ascontiguousarray(ad).view(F32).reshape(-1, 18).copy(), (b1, b2, it)


def twin_frame(tgt, s9):
    """image0 of the white twin from the oracle: [..., 0] is the coverage."""
    return CR.oracle_of(tgt, CR.white_twin(s9)).forward().copy()


def bits_check(W, H, s, tgt, kw, label, oracle=True):
    """Forward bits and deterministic backward bits of a coverage context against a plain context and the white twin, all of
    the kind `kw`.  -> (image0 of the coverage context, its gradients under (0, 0, 0, u))."""
    s9 = f9(s)
    n = len(s9)
    fp16 = bool(kw.get("fp16_images"))
    with context(W, H, s9, tgt, coverage=True, **kw) as c, context(W, H, s9, tgt, **kw) as p, \
            context(W, H, CR.white_twin(s9), tgt, **kw) as w:
        for t in (c, p, w):
            t.forward()
        ic, ip, iw = c.get_image(), p.get_image(), w.get_image()
        grads0 = c.get_grads() if n == 0 else None
    assert ic[..., :3].tobytes() == ip[..., :3].tobytes(), label
    assert (ip[..., 3] == 1).all(), label
    if n == 0:
        assert not ic.any() and grads0.shape == (0,), label
        return ic, np.zeros((0, 9), dtype=F32)
    assert ic[..., 3].tobytes() == iw[..., 0].tobytes(), label
    if oracle and not fp16:
        assert ic[..., 3].tobytes() == twin_frame(tgt, s9)[..., 0].tobytes(), label
    # backward: deterministic contexts of the same kind
    det = dict(kw, deterministic=True)
    rgb0 = (ic - (CR.fp16_round(tgt) if fp16 else tgt)).astype(F32)
    rgb0[..., 3] = 0.0
    a0 = np.zeros(ic.shape, dtype=F32)
    a0[..., 3] = CR.signed_upstream(H, W, n)
    ured = np.zeros(ic.shape, dtype=F32)
    ured[..., 0] = a0[..., 3]
    ured[..., 3] = 7.5  # (ignored by a plain context)
    with context(W, H, s9, tgt, coverage=True, **det) as c, context(W, H, s9, tgt, **det) as p:
        gc, gp = TC.backward_from(c, rgb0, False), TC.backward_from(p, rgb0, False)
    assert same_grads(gc, gp), label
    with context(W, H, s9, tgt, coverage=True, **det) as c, context(W, H, CR.white_twin(s9), tgt, **det) as w:
        gc, gw = TC.backward_from(c, a0, False), TC.backward_from(w, ured, False)
    assert same_grads(gc[:, GEOM], gw[:, GEOM]), label
    assert np.all(gc[:, COLOUR] == 0), label
    return ic, gc


# ---------------------------------------------------------------------------------------------
# C1. the adversarial sweep
# ---------------------------------------------------------------------------------------------
def sweep_kw(seed):
    v = CR.SWEEP_VARIANTS[seed % 4]
    return v, ({} if v == "plain" else {v: True})


@pytest.mark.parametrize("seed", CR.SWEEP_SEEDS)
def test_sweep_forward_and_deterministic_backward_bits(seed):
    W, H, n, s, tgt = CR.sweep_case(seed)
    v, kw = sweep_kw(seed)
    ic, gc = bits_check(W, H, s, tgt, kw, (seed, W, H, n, v))
    if n:
        assert np.isfinite(gc).all()   # (tests/test_coverage_cpu.py: the oracle's is)


@pytest.mark.parametrize("seed", CR.SWEEP_SEEDS)
def test_sweep_mixed_upstream_meets_the_two_oracle_passes(seed):
    """s2d_backward of a coverage context (the upstream image0 - target on four channels) against the two oracle passes it
    splits into, all terms summed in double: bar (a), 1e-6 of the summed |terms|, in the context kind of the seed -- float
    atomics in three of four."""
    W, H, n, s, tgt = CR.sweep_case(seed)
    v, kw = sweep_kw(seed)
    if n == 0:
        with context(W, H, s, tgt, coverage=True, **kw) as c:
            c.forward()
            c.backward(skip_opacity_grad=False)
            assert c.get_grads().shape == (0,) and not c.get_image().any()
        return
    o = CR.FourChannelOracle(tgt, s, mode="f64", fp16=(v == "fp16_images"))
    mse, _, dsum = o.gradients()
    with context(W, H, s, tgt, coverage=True, **kw) as c:
        c.forward()
        c.backward(skip_opacity_grad=False)
        g = TC.g9(c).astype(np.float64)
        got_mse = c.mse()
        cov = c.get_image()[..., 3]
    assert cov.tobytes() == o.coverage.tobytes()
    if v != "fp16_images":
        assert abs(got_mse - mse) <= 1e-9 * mse   # (three channels: the fourth does not enter)
    nz = o.dabs > 0
    assert np.all(g[~nz] == 0)
    worst = float((np.abs(g - dsum)[nz] / o.dabs[nz]).max()) if nz.any() else 0.0
    print("\n[coverage limits] sweep %d %dx%d n=%d %s: max |g - dsum| / dabs = %.3e" % (seed, W, H, n, v, worst))
    assert worst <= 1e-6, worst


# ---------------------------------------------------------------------------------------------
# C2. named edges
# ---------------------------------------------------------------------------------------------
def rgba_target(W, H):
    tgt = O.synthetic_target(W, H)
    tgt[..., 3] = CR.alpha_pattern(H, W)
    return tgt


def test_minimum_size_splats_on_pixel_centres_reach_coverage_one():
    """The scene of tests/test_gpu_parity.py::test_minimum_size_splats_and_pixel_centres: sx = sy = 1, opacity 1, positions on
    centres, corners and borders.  alpha is exactly 1 at a centre, so 1 - alpha + 1e-15 is 1e-15 in the backward walk and the
    coverage is exactly 1.0 there; whatever is not finite in the gradients is so at the twin's places."""
    W, H = 48, 32
    pts = [(x + dx, y + dy) for x in (0, 15, 16, 31, 47) for y in (0, 15, 16, 31) for dx, dy in ((0.5, 0.5), (0.0, 0.0))]
    pts = [(min(px, W - 1), min(py, H - 1)) for px, py in pts]
    n = len(pts)
    s = np.zeros(n, dtype=O.SPLAT_DTYPE)
    s["pos"] = np.array(pts, dtype=F32)
    s["sx"] = 1.0
    s["sy"] = 1.0
    s["rot"] = np.linspace(0, 3, n)
    s["color"] = np.linspace(0.1, 0.9, n)[:, None]
    s["opacity"] = 1.0
    for kw in ({}, {"fp16_images": True}):
        ic, gc = bits_check(W, H, s, rgba_target(W, H), kw, kw)
        assert (ic[..., 3] == 1.0).any() and (ic[..., 3] == 0.0).any()
        assert gc[:, GEOM].any()


def test_low_opacity_deep_stack():
    """tests/test_gpu_parity.py::test_low_opacity_deep_stacks cut to 64 x 48 with 600 splats: some 50 splats per pixel before
    the 1/256 cut-off, the coverage built from small addends."""
    W, H, n = 64, 48, 600
    rng = np.random.default_rng(22)
    s = np.zeros(n, dtype=O.SPLAT_DTYPE)
    s["pos"][:, 0] = rng.uniform(0, W - 1, n)
    s["pos"][:, 1] = rng.uniform(0, H - 1, n)
    s["sx"] = rng.uniform(4, 12, n)
    s["sy"] = rng.uniform(4, 12, n)
    s["rot"] = rng.uniform(0, np.pi, n)
    s["color"] = rng.uniform(0, 1, (n, 3))
    s["opacity"] = rng.choice([0.1, 0.15, 0.3], n)
    ic, gc = bits_check(W, H, s, rgba_target(W, H), {}, "deep stack")
    assert (ic[..., 3] > 0.99).any() and (ic[..., 3] < 1.0).all() and np.isfinite(gc).all() and gc[:, 8].any()


def test_single_row_image_and_splats_entirely_off_the_image():
    W, H = 200, 1
    s = O.random_splats(50, W, 4, 31)
    s["pos"][:, 1] = 0
    ic, gc = bits_check(W, H, s, rgba_target(W, H), {}, "200 x 1")
    assert ic[..., 3].any() and gc[:, GEOM].any()
    W, H = 64, 64
    s = O.random_splats(40, W, H, 32)
    s["pos"][:20] = [-500.0, 30.0]      # far outside on the left
    s["pos"][20:30] = [30.0, 5000.0]
    ic, gc = bits_check(W, H, s, rgba_target(W, H), {}, "off image")
    assert ic[..., 3].any() and gc[30:, GEOM].any()
    with context(W, H, s, rgba_target(W, H), coverage=True) as c:
        c.forward()
        assert c.stats()["pairs_binned"] < 40 * 16


STRIP = (8208, 32, 1500, 41)   # 513 tile columns: the generic builder, chosen by the library


@functools.lru_cache(maxsize=None)
def strip():
    W, H, n, seed = STRIP
    s = O.random_splats(n, W, H, seed)
    tgt = rgba_target(W, H)
    s.setflags(write=False)
    tgt.setflags(write=False)
    return s, tgt


def test_strip_wider_than_512_tile_columns():
    """Beyond 8192 pixels of width the library takes the generic list builder on its own; splats from one tile to 1024 px,
    tile retirement and the hand-over after it across 513 tile columns."""
    W, H, n, _ = STRIP
    s, tgt = strip()
    ic, gc = bits_check(W, H, s, tgt, {}, "strip")
    assert (ic[..., 3] == 0).any() and (ic[..., 3] > 0.99).any() and gc[:, GEOM].any()
    with context(W, H, s, tgt, coverage=True) as c:
        c.forward()
        assert c.stats()["pairs_binned"] > n
        c.backward()
        assert TC.g9(c).any() and np.isfinite(c.step(1)).all()   # ... and the context still answers


def test_view_of_the_strip_wider_than_8192_output_pixels():
    """A view's lists are built for the output size: 8240 output pixels, 515 tile columns, the view's generic builder with the
    coverage flag."""
    W, H, n, _ = STRIP
    s, tgt = strip()
    view = dict(out_width=8240, out_height=24, origin=(3.25, 2.5), zoom=1.004, samples=1)
    for rgba8 in (False, True):
        with context(W, H, s, tgt, coverage=True) as c, context(W, H, s, tgt) as p, context(W, H, CR.white_twin(s), tgt) as w:
            vc, vp, vw = (t.render_view(rgba8=rgba8, **view) for t in (c, p, w))
        assert vc[..., :3].tobytes() == vp[..., :3].tobytes() and vp[..., :3].any()
        assert vc[..., 3].tobytes() == vw[..., 0].tobytes()
        assert len(np.unique(vc[..., 3])) > 10 and (vp[..., 3] == (255 if rgba8 else 1)).all()
        assert vc[:, 8192:, 3].any()   # (the columns beyond the two-level builder's reach are drawn)


# ---------------------------------------------------------------------------------------------
# C3. training against the CPU loop
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opacity", [False, True], ids=["fixed_opacity", "optimize_opacity"])
@pytest.mark.parametrize("name", CR.SCENES)
def test_five_steps_follow_the_four_channel_loop_of_the_oracle(name, opacity):
    """s2d_step in a coverage context with float atomics against coverage_ref.FourChannelOracle("f32"), with the bars of
    tests/test_gpu_parity.py::test_training_steps_random_sweep: the MSE of iteration 0 to 1e-9 (the same framebuffer), the
    later ones to 2e-5, the parameters after five steps to 5 * 1e-3 * lr + 1e-5 * max |ref|.
    Measured (MI355X): see DESIGN.md section 22."""
    CR.assert_scenes_are_not_trivial()
    want, ref = CR.five_steps(name, opacity, "f32")
    with TC.make(name, coverage=True) as c:
        c.optimize_opacity = opacity
        got = c.step(5)
        sp = f9(c.get_splats()).astype(np.float64)
        assert c.get_adam()[3] == 5
    bar = CR.update_bar(ref)
    worst = float(np.abs(sp - ref).max())
    print("\n[coverage limits] %s opacity=%s: mse rel %s; max |gpu - ref| after 5 steps %.3e, bar %.3e"
          % (name, opacity, " ".join("%.1e" % r for r in np.abs(got - want) / want), worst, bar))
    assert abs(got[0] - want[0]) <= 1e-9 * want[0]
    np.testing.assert_allclose(got, want, rtol=2e-5)
    assert worst <= bar, (worst, bar)


# ---------------------------------------------------------------------------------------------
# C4. the combinations section 22 claims
# ---------------------------------------------------------------------------------------------
ALIVE_CASES = [("mini", m) for m in ("one", "every_second", "first_block_dead", "last_20", "random_half")] + \
              [("stack", m) for m in ("every_second", "last_20", "random_half")]


@pytest.mark.parametrize("name,mask_name", ALIVE_CASES)
def test_alive_set_five_deterministic_steps_equal_the_compact_context(name, mask_name):
    """A coverage context with a mask against a coverage context that holds only the alive rows (the construction of
    tests/test_gpu_alive.py::test_five_deterministic_steps_equal_the_compact_context_bytewise): bytes, under dead rows too."""
    tgt, s9 = CR.scene(name)
    H, W = tgt.shape[:2]
    alive = AR.masks(len(s9))[mask_name]
    assert alive.any() and not alive.all()
    with context(W, H, s9, tgt, coverage=True, deterministic=True) as t, \
            context(W, H, AR.compact(s9, alive), tgt, coverage=True, deterministic=True) as c:
        t.set_alive(alive)
        t.optimize_opacity = c.optimize_opacity = True
        before = state(t)
        mse_t, mse_c = t.step(5), c.step(5)
        after, compact = state(t), state(c)
        img_t, img_c = t.get_image(), c.get_image()
        t.forward()
        now_t = t.get_image()
        t.backward(skip_opacity_grad=False)
        c.forward()
        c.backward(skip_opacity_grad=False)
        g_t, g_c = TC.g9(t), TC.g9(c)
        assert t.alive()[0].tolist() == alive.tolist()
    # ... and independent of the library: the oracle's twin on the alive rows, in their order
    assert now_t[..., 3].tobytes() == twin_frame(tgt, after[0][alive])[..., 0].tobytes() and now_t[..., 3].any()
    assert mse_t.tobytes() == mse_c.tobytes() and after[2] == compact[2]
    assert after[0].tobytes() == AR.expand(compact[0], alive, before[0]).tobytes()      # dead rows keep their 27 floats
    assert after[1].tobytes() == AR.expand(compact[1], alive, before[1]).tobytes()
    assert (after[0][alive] != before[0][alive]).any()
    assert img_t.tobytes() == img_c.tobytes() and img_t[..., 3].any()
    assert not g_t[~alive].view(np.uint32).any()                                        # +0, every bit
    assert same_grads(g_t[alive], g_c) and g_c[:, GEOM].any()


def test_group_rates_and_a_frozen_mask_after_a_coverage_backward():
    """One adam_step under s2d_set_optim and s2d_set_frozen equals the composite oracle of tests/optim_ref.py applied to the
    coverage context's own gradients, every bit; frozen rows are byte-identical."""
    tgt, s9 = CR.scene("mini")
    H, W = tgt.shape[:2]
    n = len(s9)
    frozen = np.zeros(n, dtype=bool)
    frozen[::3] = True
    with context(W, H, s9, tgt, coverage=True, deterministic=True) as t:
        t.optimize_opacity = True
        t.set_optim(pos=.5, scale=.2, rot=.1, color=.05, opacity=.05)
        t.set_frozen(frozen)
        t.step(2)                                   # moments and beta words away from their initial values
        t.forward()
        t.backward(skip_opacity_grad=False)
        g = TC.g9(t)
        s0, a0, (b1, b2, it) = state(t)
        rates = t.rates_at(it)
        t.adam_step()
        s1, a1, (c1, c2, it1) = state(t)
    assert it == 2 and it1 == 3 and g[:, GEOM].any() and g[:, COLOUR].any()
    assert rates.tolist() == [F32(.5), F32(.2), F32(.1), F32(.05), F32(.05)]
    o = OR.CompositeState(s0, a0.reshape(-1, 9, 2), W, H, b1, b2, it)
    assert o.step(g, True, rates, frozen) == 0
    A.assert_same_bits(s1, o.splats, "parameters")
    A.assert_same_bits(a1.reshape(-1, 9, 2), o.adams, "moments")
    assert (c1, c2) == (o.beta1t[0], o.beta2t[0])
    assert s1[frozen].tobytes() == s0[frozen].tobytes() and a1[frozen].tobytes() == a0[frozen].tobytes()
    assert (s1[~frozen] != s0[~frozen]).any() and (s1[~frozen][:, 8] != s0[~frozen][:, 8]).any()


def test_adam_fp32_step_after_a_coverage_backward():
    """S2D_CFG_ADAM_FP32 with the coverage flag: one step equals the oracle's rule in that mode (s2do_set_adam_fp32, as
    tests/test_gpu_parity.py::test_adam_fp32_quotient_mode_matches_the_oracle_in_that_mode switches it) applied to the
    context's own gradients, every bit -- and not the rule of the default mode."""
    tgt, s9 = CR.scene("mini")
    H, W = tgt.shape[:2]
    with context(W, H, s9, tgt, coverage=True, deterministic=True, adam_fp32=True) as t:
        t.step(2)
        t.forward()
        t.backward(skip_opacity_grad=False)
        g = TC.g9(t)
        s0, a0, (b1, b2, it) = state(t)
        t.adam_step()
        s1, a1, (c1, c2, it1) = state(t)
    o = A.OracleState(s0, a0.reshape(-1, 9, 2), W, H, b1, b2, it, fp32=True)
    assert o.step(g, False) == 0
    A.assert_same_bits(s1, o.splats, "parameters")
    A.assert_same_bits(a1.reshape(-1, 9, 2), o.adams, "moments")
    assert (c1, c2) == (o.beta1t[0], o.beta2t[0]) and it1 == 3
    d = A.OracleState(s0, a0.reshape(-1, 9, 2), W, H, b1, b2, it, fp32=False)
    assert d.step(g, False) == 0 and (A.bits(d.splats) != A.bits(o.splats)).any()


def fresh_forward(W, H, s9, tgt):
    """image0 of a fresh coverage context given the splats, and image0 of their white twin in a plain context."""
    with context(W, H, s9, tgt, coverage=True) as c, context(W, H, CR.white_twin(s9), tgt) as w:
        c.forward()
        w.forward()
        return c.get_image(), w.get_image()


def test_seed_and_grow_leave_a_context_that_renders_like_a_fresh_one():
    W, H, n = 96, 80, 300
    tgt = rgba_target(W, H)
    s = O.random_splats(n, W, H, 14)
    with context(W, H, s, tgt, coverage=True) as t:
        t.forward()                                  # lists of the old splats exist
        old = t.get_image()
        assert t.seed(source="edges", seed=5, scale=2.5) == n
        t.forward()
        got, sp = t.get_image(), f9(t.get_splats()).copy()
    want, twin = fresh_forward(W, H, sp, tgt)
    assert (sp != f9(s)).any() and got.tobytes() != old.tobytes()
    assert got.tobytes() == want.tobytes() and got[..., 3].tobytes() == twin[..., 0].tobytes() and got[..., 3].any()
    alive = np.zeros(n, dtype=bool)
    alive[n - 50:] = True
    with context(W, H, s, tgt, coverage=True) as t:
        t.set_alive(alive)
        t.step(2)
        t.forward()
        old = t.get_image()
        assert t.grow(40, source="error", squared=True, seed=5, scale=2.5) == 40
        now, count = t.alive()
        assert count == 90 and now[:40].all() and not now[40:n - 50].any()
        t.forward()
        got, sp = t.get_image(), f9(t.get_splats()).copy()
    want, twin = fresh_forward(W, H, AR.compact(sp, now), tgt)
    assert got.tobytes() != old.tobytes()
    assert got.tobytes() == want.tobytes() and got[..., 3].tobytes() == twin[..., 0].tobytes() and got[..., 3].any()


@pytest.mark.parametrize("lr", [0.0, 4.0])
def test_reused_tile_lists_stay_exact_under_the_separate_launches_of_step(lr):
    """The construction of tests/test_gpu_parity.py::test_cached_tile_lists_stay_exact with rebin_interval = 8, driven by
    s2d_step (forward, backward and Adam as separate launches in a coverage context): the frame of every iteration is that of
    the oracle, and its .w that of the oracle's twin, run on the splats the context held before the step.  lr = 4 moves
    splats far outside the binning margin: the containment check must force rebuilds."""
    tgt = CR.scene("mini")[0]
    H, W = tgt.shape[:2]
    n = CR.N_MINI
    with S2D.Trainer(W, H, n, rebin_interval=8, training_rate=lr, coverage=True) as t:
        t.set_target(tgt)
        t.init()
        for k in range(24):
            s9 = f9(t.get_splats()).copy()
            assert np.isfinite(t.step(1)).all()
            img = t.get_image()
            assert img[..., 3].tobytes() == twin_frame(tgt, s9)[..., 0].tobytes(), k
            if k % 8 == 7:
                assert img[..., :3].tobytes() == CR.oracle_of(tgt, s9).forward()[..., :3].tobytes(), k
        st = t.stats()
    if lr == 0.0:
        assert st["rebins"] < 24 // 2   # lists really were re-used
    else:
        assert st["rebins"] > 24 // 8   # unscheduled rebuilds happened


def test_nonfinite_guard_reports_status_and_stops_the_queue():
    """tests/test_gpu_parity.py::test_nonfinite_guard_reports_status and ::test_nonfinite_stops_the_queue_where_the_reference_aborts
    in a coverage context, where the iterations of s2d_step are three launches each: status 3, the iteration, NaN for the MSE of
    what never ran, nothing moved afterwards, and new parameters clear the condition."""
    with S2D.Trainer(32, 32, 8, coverage=True) as t:
        t.set_target(rgba_target(32, 32))
        t.init()
        s = t.get_splats()
        s["rot"][3] = np.nan
        t.set_splats(s)
        with pytest.raises(S2D.S2DError) as ei:
            t.step(1)
        assert ei.value.code == 3  # S2D_E_NONFINITE
        assert t.stats()["first_nonfinite_iteration"] == 0
    tgt = CR.scene("mini")[0]
    H, W = tgt.shape[:2]
    n = 500
    with S2D.Trainer(W, H, n, coverage=True) as t:
        t.set_target(tgt)
        t.init()
        t.step(3)
        ad, b1, b2, it = t.get_adam()
        assert it == 3
        ad["mv"][7, 4, 0] = np.inf  # first moment of splat 7's rot: its next update is non-finite
        t.set_adam(ad, b1, b2, it)
        mse = np.zeros(6)
        rc = t.L.s2d_step(t._h, 6, 0, mse.ctypes.data_as(C.c_void_p))
        assert rc == 3
        assert t.stats()["first_nonfinite_iteration"] == 3
        assert np.isfinite(mse[0]) and np.isnan(mse[1:]).all()   # iteration 3 printed, 4.. never ran
        s_fail = t.get_splats()
        assert not np.isfinite(s_fail["rot"][7])
        with pytest.raises(S2D.S2DError) as ei:
            t.step(2)                                             # still stopped ...
        assert ei.value.code == 3
        assert t.get_splats().tobytes() == s_fail.tobytes()       # ... and nothing moved
        ad2, b1f, b2f, itf = t.get_adam()
        assert itf == 4
        s_fail["rot"][7] = 0.0
        ad2["mv"][7, 4, :] = 0.0
        t.set_splats(s_fail)
        t.set_adam(ad2, b1f, b2f, itf)
        assert np.isfinite(t.step(2)).all()
        t.forward()
        img, sp = t.get_image(), f9(t.get_splats()).copy()
    assert img[..., 3].tobytes() == twin_frame(tgt, sp)[..., 0].tobytes()   # and the channel is what it should be afterwards


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
def test_image_rows_on_the_device_are_get_image(fp16):
    torch = TC._torch()
    tgt = CR.scene("mini")[0]
    H, W = tgt.shape[:2]
    buf = torch.full((H, W, 4), 7.5, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with TC.make("mini", coverage=True, fp16_images=fp16) as c:
        c.forward()
        c.get_image_rows_device(buf.data_ptr())
        c.synchronize()
        img = c.get_image()
    got = buf.cpu().numpy()
    if not fp16:
        assert got[..., 3].tobytes() == CR.oracle_frames("mini")[1][..., 0].tobytes()
    assert got.tobytes() == img.tobytes() and len(np.unique(img[..., 3])) > 10 and not (got == 7.5).any()


def test_checkpoint_round_trip_resumes_identically():
    """get_splats / get_adam into a second coverage context: the same image0, .w included, and the same next steps."""
    name = "mini"
    with TC.make(name, coverage=True, deterministic=True) as a, TC.make(name, coverage=True, deterministic=True) as b:
        a.optimize_opacity = b.optimize_opacity = True
        a.step(7)
        sp, (ad, b1, b2, it) = a.get_splats(), a.get_adam()
        a.forward()
        img_a = a.get_image()
        mse_a = a.step(3)
        b.set_splats(sp)
        b.set_adam(ad, b1, b2, it)
        b.forward()
        assert b.get_image().tobytes() == img_a.tobytes() and img_a[..., 3].any()
        assert img_a[..., 3].tobytes() == twin_frame(CR.scene(name)[0], f9(sp))[..., 0].tobytes()
        mse_b = b.step(3)
        assert b.stats()["iterations"] == 10
        assert mse_a.tobytes() == mse_b.tobytes() and a.get_splats().tobytes() == b.get_splats().tobytes()
        assert a.get_image().tobytes() == b.get_image().tobytes()


# ---------------------------------------------------------------------------------------------
# C5. the host program
# ---------------------------------------------------------------------------------------------
def disc_png():
    """64 x 48 RGBA8: an opaque disc with a soft edge, and a transparent region that still carries colour bytes."""
    W, H = 64, 48
    y, x = np.mgrid[0:H, 0:W]
    r = np.sqrt((x + 0.5 - 30.0) ** 2 + (y + 0.5 - 25.0) ** 2)
    a = np.clip((18.0 - r) / 5.0, 0.0, 1.0)                   # 1 inside 13 px, 0 beyond 18 px
    px = np.zeros((H, W, 4), dtype=np.uint8)
    px[..., 0] = 40 + 3 * x
    px[..., 1] = 200 - 2 * y
    px[..., 2] = (7 * x + 5 * y) % 256                        # colour everywhere, also where alpha is 0
    px[..., 3] = np.round(a * 255.0)
    assert (px[..., 3] == 255).any() and (px[..., 3] == 0).any() and len(np.unique(px[..., 3])) > 20
    assert px[px[..., 3] == 0][:, :3].any()
    return px


def test_host_program_trains_on_an_rgba_png_and_writes_straight_alpha(tmp_path):
    """splat2d_train --coverage against a Trainer given the premultiplied target (the formula of
    tests/test_coverage_cpu.py::test_the_coverage_target_is_premultiplied_and_the_output_is_straight): the printed trace to its
    digits, the checkpoint's splats to the byte, --out-image and the --out-size view through coverage_ref.straight_rgba8 (which
    tests/test_coverage_cpu.py holds to s2dio::quantise_straight) to the byte."""
    from PIL import Image
    exe = S2D._build.build_host_program()
    px = disc_png()
    H, W = px.shape[:2]
    png, out, view, ck = (str(tmp_path / f) for f in ("t.png", "o.png", "v.png", "ck"))
    Image.fromarray(px).save(png)
    al = px[..., 3].astype(F32) / F32(255.0)
    tgt = np.empty(px.shape, dtype=F32)
    tgt[..., :3] = (px[..., :3].astype(F32) / F32(255.0)) * al[..., None]
    tgt[..., 3] = al
    n, iters = 256, 12
    with S2D.Trainer(W, H, n, coverage=True, deterministic=True) as t:
        t.set_target(tgt)
        t.init()
        mse = t.step(iters)
        sp = t.get_splats()
        t.forward()
        image0 = t.get_image()
        v8 = t.render_view(32, 24, rgba8=True)
    base = [exe, "--image", png, "--coverage", "--deterministic", "--splats", str(n), "--iters", str(iters)]
    r = subprocess.run(base + ["--out-image", out, "--save-checkpoint", ck], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-1500:]
    assert r.stdout.strip().splitlines() == ["%d itr, mse %.4f" % (k, m) for k, m in enumerate(mse)]
    assert mse[-1] < mse[0]
    raw = open(ck, "rb").read()
    assert raw[:4] == b"S2DC" and len(raw) == 28 + n * (36 + 72)
    assert raw[28:28 + n * 36] == sp.tobytes()
    im = Image.open(out)
    assert im.mode == "RGBA" and im.size == (W, H)
    want = CR.straight_rgba8(image0)
    assert np.asarray(im).tobytes() == want.tobytes()
    opaque = image0.copy()
    opaque[..., 3] = 1.0
    assert (want[..., 3] < 255).any() and (want[..., :3] != CR.straight_rgba8(opaque)[..., :3]).any()   # (the division is at work)
    r = subprocess.run(base + ["--out-image", view, "--out-size", "32x24"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-1500:]
    im = Image.open(view)
    assert im.mode == "RGBA" and im.size == (32, 24)
    want = CR.straight_rgba8(v8.astype(F32) / F32(255.0))
    assert np.asarray(im).tobytes() == want.tobytes() and want[..., 3].any()
