"""GPU tests of density control: the statistics the backward walk gathers with S2D_BWD_DENSITY_STATS, and s2d_relocate.

Yardsticks, none of them written for this feature:
  * abs_dpos against `dabs[:, 0:2]` of the oracle's backward pass (s2do_backward_rows_stats: the reference's own per-pixel
    position addends, magnitudes summed in double), under bar (a) of oracle_lib.grad_bars: |got - want| <= 1e-6 * want, and
    exactly 0 where the oracle has no term;
  * weight against `dsum[:, 5]` (dSplats.color.x) of an oracle backward pass whose target is the pseudo-target of the
    upstream gradient (1, 0, 0) (tests/test_image_grads_cpu.py): sum of dL_r * T * alpha with dL_r = 1 to one rounding of the
    pseudo-target, i.e. 2 ulp per non-negative term: bar 1e-6 + 2^-22;
  * the gradients, the framebuffer and the squared error of the passes without the flag;
  * the planner of csrc/s2d_density.h, compiled for the host (tests/test_density_plan_cpu.py, where it is held to a NumPy
    restatement), for what s2d_relocate writes.
Measured maxima over all 38 comparisons with the oracle below (MI355X): abs_dpos 3.15e-7 (mini, float atomics), weight 2.75e-7
(mini, deterministic); every case prints its own.
"""
import functools
import importlib
import math
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import test_density_plan_cpu as DP
import test_image_grads_cpu as IG

pytestmark = pytest.mark.gpu

S2D = importlib.import_module("2dgaussiansplatting_amd")
D = importlib.import_module("2dgaussiansplatting_amd.distributed")
MINI = os.path.join(O.GOLDEN, "squirrel_cls_mini_268x213.s2di")
BAR_ABS = 1e-6                      # bar (a) of oracle_lib.grad_bars
BAR_WEIGHT = 1e-6 + 2.0 ** -22      # ... + the oracle's dL_r = 1 to 2 ulp
RANDOM_SCENES = {"33x17": (33, 17, 200, 11), "96x80": (96, 80, 300, 12), "40x1": (40, 1, 30, 13)}
SCENES = sorted(RANDOM_SCENES) + ["mini"]


def _fp16(a):
    return a.astype(np.float16).astype(np.float32)


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> (target, splats): explicit random splats (sx, sy in [1, 6], rot over a full turn, opacity in [0.1, 1]) on the
    synthetic target, or the squirrel mini with 1024 splats after 5 oracle steps."""
    if name == "mini":
        tgt = O.target_rgba32f(O.load_s2di(MINI))
        o = O.OracleTrainer(tgt, 1024)
        for _ in range(5):
            o.step()
        return tgt, o.splats.copy()
    W, H, n, seed = RANDOM_SCENES[name]
    rng = np.random.default_rng(seed)
    s = np.zeros(n, dtype=O.SPLAT_DTYPE)
    s["pos"][:, 0] = rng.uniform(0, W - 1, n)
    s["pos"][:, 1] = rng.uniform(0, H - 1, n)
    s["sx"] = rng.uniform(1.0, 6.0, n)
    s["sy"] = rng.uniform(1.0, 6.0, n)
    s["rot"] = rng.uniform(-np.pi, np.pi, n)
    s["color"] = rng.uniform(0, 1, (n, 3))
    s["opacity"] = rng.uniform(0.1, 1.0, n)
    return O.synthetic_target(W, H), s


def _weight_from(o):
    """sum T * alpha per splat from the oracle: dSplats.color.x under dL/dC = (1, 0, 0), image0 as the oracle holds it."""
    g = np.zeros_like(o.image0)
    g[..., 0] = 1.0
    keep = o.ref
    o.ref = np.ascontiguousarray(IG.pseudo_target(o.image0, g))
    try:
        return o.backward_stats()[1][:, 5].copy()
    finally:
        o.ref = keep


@functools.lru_cache(maxsize=None)
def oracle_stats(name, fp16=False):
    """Oracle side of a scene, computed once: {"abs": (n, 2), "weight": (n,), "image": image0}.  fp16: the oracle on a
    target and a framebuffer rounded to fp16, as test_fp16_images_match_the_oracle_with_rounded_images runs it."""
    tgt, splats = scene(name)
    o = O.OracleTrainer(_fp16(tgt) if fp16 else tgt, len(splats))
    o.splats[:] = splats
    o.forward()
    if fp16:
        o.image0[:] = _fp16(o.image0)
    dabs = o.backward_stats()[2]
    return {"abs": dabs[:, 0:2].copy(), "weight": _weight_from(o), "image": o.image0.copy()}


@functools.lru_cache(maxsize=None)
def oracle_upstream(name):
    """A signed, masked upstream gradient (the weighted Charbonnier loss of test_image_grads_cpu) and the oracle's sum of
    |position addends| under its pseudo-target: (upstream as the oracle forms it, abs (n, 2))."""
    tgt, splats = scene(name)
    o = O.OracleTrainer(tgt, len(splats))
    o.splats[:] = splats
    img = o.forward().copy()
    g = IG.charbonnier_grad(img, tgt, IG.charbonnier_weights(*tgt.shape[:2]))
    pseudo = IG.pseudo_target(img, g)
    o.ref = np.ascontiguousarray(pseudo)
    dabs = o.backward_stats()[2]
    up = IG.upstream_of(img, pseudo)
    assert (up[..., :3] < 0).any() and (up[..., :3] > 0).any()
    return up, dabs[:, 0:2].copy()


def trainer(name, **kw):
    tgt, splats = scene(name)
    t = S2D.Trainer(tgt.shape[1], tgt.shape[0], len(splats), **kw)
    t.set_target(tgt)
    t.set_splats(splats.view(S2D.SPLAT_DTYPE))
    return t


def rel_err(got, want):
    """max |got - want| / want where want > 0; asserts exact zeros where want is 0."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    nz = want > 0
    assert np.all(got[~nz] == 0)
    return float((np.abs(got - want)[nz] / want[nz]).max()) if nz.any() else 0.0


def check_against_oracle(label, stats, want_abs, want_weight=None):
    e_abs = rel_err(stats[:, 0:2], want_abs)
    e_w = rel_err(stats[:, 2], want_weight) if want_weight is not None else 0.0
    print("\n[density] %s: abs_dpos %.3e (bar %.1e), weight %.3e (bar %.3e), %d of %d splats without a term"
          % (label, e_abs, BAR_ABS, e_w, BAR_WEIGHT, int((want_abs.sum(axis=1) == 0).sum()), len(want_abs)))
    assert e_abs <= BAR_ABS, e_abs
    assert e_w <= BAR_WEIGHT, e_w


VARIANTS = {"default": ({}, False), "deterministic": ({"deterministic": True}, False), "fp16_images": ({"fp16_images": True}, False),
            "generic_binning": ({"generic_binning": True}, False), "no_opacity_grad": ({}, True),
            "deterministic_no_opacity_grad": ({"deterministic": True}, True),
            "deterministic_fp16_images": ({"deterministic": True, "fp16_images": True}, False)}


# ---------------------------------------------------------------------------------------------
# 1. the statistics against the oracle
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("name", SCENES)
def test_statistics_match_the_oracles_per_pixel_terms(name, variant):
    kw, skip = VARIANTS[variant]
    ref = oracle_stats(name, bool(kw.get("fp16_images")))
    with trainer(name, **kw) as t:
        assert t.density()[1] == 0 and not t.density()[0].any()      # before any statistics pass: zeros, 0 passes
        t.forward()
        assert t.get_image().tobytes() == ref["image"].tobytes()
        t.backward(skip_opacity_grad=skip, density_stats=True)
        stats, passes = t.density()
        assert passes == 1 and stats.shape == (t.n, 3)
        if skip:
            assert not t.get_grads()["opacity"].any()
    check_against_oracle("%s / %s" % (name, variant), stats, ref["abs"], ref["weight"])
    assert (ref["weight"] > 0).any()


@pytest.mark.parametrize("deterministic", [False, True], ids=["atomic", "deterministic"])
@pytest.mark.parametrize("name", SCENES)
def test_statistics_of_the_upstream_entry_point(name, deterministic):
    """s2d_backward_image_grads with the flag, from a signed masked upstream: abs_dpos against the oracle on its
    pseudo-target (the weight does not depend on the loss at all: it must be what s2d_backward gathers)."""
    import torch
    up, want_abs = oracle_upstream(name)
    ref = oracle_stats(name)
    with trainer(name, deterministic=deterministic) as t:
        t.forward()
        u = torch.from_numpy(np.ascontiguousarray(up)).cuda()
        torch.cuda.synchronize()
        t.backward_image_grads(u.data_ptr(), skip_opacity_grad=False, density_stats=True)
        stats, passes = t.density()
        assert passes == 1
        out = torch.empty((t.n, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        assert t.density_device(out.data_ptr()) == 1
        t.synchronize()
        assert out.cpu().numpy().tobytes() == stats.tobytes()       # the device getter returns the same bytes
    check_against_oracle("%s / upstream, deterministic=%s" % (name, deterministic), stats, want_abs, ref["weight"])


# ---------------------------------------------------------------------------------------------
# 2. gradients unchanged, accumulation, slabs
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("skip", [False, True], ids=["opacity", "skip_opacity"])
@pytest.mark.parametrize("name", ["96x80", "mini"])
def test_gradients_are_byte_identical_with_and_without_the_flag(name, skip):
    out = []
    for flag in (False, True):
        with trainer(name, deterministic=True) as t:
            t.forward()
            t.backward(skip_opacity_grad=skip, density_stats=flag)
            out.append((t.get_grads().tobytes(), t.mse(), t.density()[1]))
    assert out[0][0] == out[1][0] and np.frombuffer(out[0][0], dtype=np.float32).any()
    assert out[0][1] == out[1][1] and (out[0][2], out[1][2]) == (0, 1)


@pytest.mark.parametrize("deterministic", [True, False], ids=["deterministic", "atomic"])
def test_statistics_accumulate_over_passes_and_reset(deterministic):
    def one_pass(t):
        t.forward()
        t.backward(density_stats=True)
        return t.density()

    with trainer("96x80", deterministic=deterministic) as t:
        d1, p1 = one_pass(t)
        t.backward(density_stats=True)      # unchanged parameters: the same terms once more
        d2, p2 = t.density()
        assert (p1, p2) == (1, 2) and d1.any()
        t.backward()                        # a pass without the flag neither counts nor adds
        assert t.density()[0].tobytes() == d2.tobytes() and t.density()[1] == 2
        t.density_reset()
        d0, p0 = t.density()
        assert p0 == 0 and not d0.any()
        d3, p3 = one_pass(t)                # ... and the buffer starts again from zero
        t.init()                            # s2d_init_splats resets the statistics
        assert t.density()[1] == 0 and not t.density()[0].any()
    with trainer("96x80", deterministic=deterministic) as fresh:
        df, _ = one_pass(fresh)
        fresh.set_splats(scene("96x80")[1].view(S2D.SPLAT_DTYPE))   # s2d_set_splats does not reset them
        assert fresh.density()[1] == 1 and fresh.density()[0].tobytes() == df.tobytes()
    if deterministic:
        assert d2.tobytes() == (d1 + d1).tobytes() and df.tobytes() == d1.tobytes() and d3.tobytes() == d1.tobytes()
    else:
        for got, want in ((d2, 2.0 * d1.astype(np.float64)), (df, d1), (d3, d1)):
            e = rel_err(got, want)
            print("\n[density] atomic accumulation: %.3e" % e)
            assert e <= BAR_ABS


def test_slab_contexts_add_up_to_the_whole_image():
    ref = oracle_stats("96x80")
    with trainer("96x80") as full:
        full.forward()
        full.backward(density_stats=True)
        whole = full.density()[0].astype(np.float64)
    parts = np.zeros_like(whole)
    for rank in range(2):
        r0, r1 = D.slab_rows(80, rank, 2)
        with trainer("96x80", row_begin=r0, row_end=r1) as t:
            t.forward()
            t.backward(density_stats=True)
            part = t.density()[0]
            assert part.any() and (part >= 0).all()
            parts += part
    e = rel_err(parts, whole)
    print("\n[density] two slabs against the whole image: %.3e" % e)
    assert e <= BAR_ABS
    check_against_oracle("96x80 / two slabs", parts, ref["abs"], ref["weight"])


# ---------------------------------------------------------------------------------------------
# 3. s2d_step with the flag
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mini_state():
    tgt = O.target_rgba32f(O.load_s2di(MINI))
    o = O.OracleTrainer(tgt, 2000)
    for _ in range(3):
        o.step()
    return tgt, o.splats.copy(), o.adams.copy(), float(o.beta1t[0]), float(o.beta2t[0]), o.iterations


def mini_trainer(**kw):
    tgt, splats, adams, b1, b2, it = mini_state()
    t = S2D.Trainer(tgt.shape[1], tgt.shape[0], 2000, **kw)
    t.set_target(tgt)
    t.set_splats(splats.view(S2D.SPLAT_DTYPE))
    t.set_adam(adams.view(S2D.ADAM_DTYPE), b1, b2, it)
    return t


@pytest.mark.parametrize("kw", [{}, {"deterministic": True}, {"fp16_images": True}, {"deterministic": True, "fp16_images": True}])
def test_step_with_the_flag_equals_the_plain_step(kw):
    """What test_fused_forward_backward_equals_the_two_passes holds the fused launch to against the separate calls --
    identical framebuffer, identical squared error, gradients bitwise with deterministic sums and within 1e-5 of the
    component's largest magnitude with float atomics -- between the fused launch and forward + backward WITH the flag; and
    5 iterations of s2d_step either way.  With deterministic sums the 5 iterations are bytes-equal throughout.  With float
    atomics two runs of the same code already differ after the first Adam step, so there iteration 0 (identical parameters)
    is held to identical squared error and the later ones to 2e-5 of the MSE, the bar of smoke() for one iteration."""
    res = []
    for flag in (False, True):
        with mini_trainer(**kw) as t:
            if flag:
                t.forward()
                t.backward(density_stats=True)
            else:
                t.forward_backward()
            res.append((t.get_image(), t.get_grads().view(np.float32).reshape(-1, 9).copy(), t.mse()))
    (img_a, g_a, m_a), (img_b, g_b, m_b) = res
    assert img_a.tobytes() == img_b.tobytes() and m_a == m_b
    if kw.get("deterministic"):
        assert g_a.tobytes() == g_b.tobytes()
    else:
        scale = np.abs(g_a).max(axis=0) + 1e-30
        assert (np.abs(g_a - g_b) / scale).max() <= 1e-5
    runs = []
    for flag in (False, True):
        with mini_trainer(**kw) as t:
            mse = t.step(5, density_stats=flag)
            runs.append((mse, t.get_image(), t.get_splats(), t.get_adam(), t.density()))
    (mse_a, im_a, s_a, ad_a, d_a), (mse_b, im_b, s_b, ad_b, d_b) = runs
    assert d_a[1] == 0 and d_b[1] == 5 and d_b[0].any() and not d_a[0].any()
    assert ad_a[1:] == ad_b[1:] and ad_b[3] == 8                      # beta powers and iteration count
    assert mse_a[0] == mse_b[0] and np.isfinite(mse_b).all()
    if kw.get("deterministic"):
        assert mse_a.tobytes() == mse_b.tobytes() and im_a.tobytes() == im_b.tobytes()
        assert s_a.tobytes() == s_b.tobytes() and ad_a[0].tobytes() == ad_b[0].tobytes()
    else:
        assert (np.abs(mse_a - mse_b) <= 2e-5 * mse_a).all(), (mse_a, mse_b)
        assert np.isfinite(s_b.view(np.float32)).all()


# ---------------------------------------------------------------------------------------------
# 4. status codes
# ---------------------------------------------------------------------------------------------
def _code(call):
    with pytest.raises(S2D.S2DError) as e:
        call()
    return e.value.code


def test_status_codes():
    import torch
    tgt, splats = scene("96x80")
    u = torch.zeros((80, 96, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with trainer("96x80") as t:
        t.forward()
        assert t.L.s2d_forward_backward(t._h, S2D.S2D_BWD_DENSITY_STATS) == 1       # no fused variant
        assert t.density()[1] == 0
        assert _code(lambda: t.relocate(5, 1.0)) == 5                                # no statistics pass yet
        t.backward(density_stats=True)
        for bad in (lambda: t.relocate(-1, 1.0), lambda: t.relocate(5, float("nan")), lambda: t.relocate(5, 1.0, shrink=-2.0)):
            assert _code(bad) == 1
        assert t.L.s2d_relocate(t._h, None, None) == 1
        cfg = S2D._RelocateConfig(4, 5, 1.0, 0.0)                                    # a struct of another size
        assert t.L.s2d_relocate(t._h, cfg, None) == 1
        assert t.density()[1] == 1                                                   # refused calls changed nothing
        t.density_reset()
        assert _code(lambda: t.relocate(5, 1.0)) == 5                                # ... nor after a reset
    for kw in ({"count_pairs": True}, {"exact_exp": True}, {"reference_order": True}):
        with trainer("96x80", **kw) as t:
            t.forward()
            assert _code(lambda: t.backward(density_stats=True)) == 1, kw
            assert _code(lambda: t.backward_image_grads(u.data_ptr(), density_stats=True)) == 1, kw
            assert _code(lambda: t.step(1, density_stats=True)) == 1, kw
            assert t.density()[1] == 0
            t.forward()
            t.backward()                                                             # the context still works without the flag
    with trainer("96x80", reference_order=True) as t:
        assert _code(lambda: t.relocate(5, 1.0)) == 1
    with trainer("96x80", chunk_pairs=700) as t:                                     # rendered by index ranges
        t.forward()
        assert _code(lambda: t.backward(density_stats=True)) == 4
        assert _code(lambda: t.backward_image_grads(u.data_ptr(), density_stats=True)) == 4
        assert _code(lambda: t.step(1, density_stats=True)) == 4
        assert t.density()[1] == 0
        t.forward()
        t.backward()
    r0, r1 = D.slab_rows(80, 1, 2)
    with trainer("96x80", row_begin=r0, row_end=r1) as t:                            # a slab context
        t.forward()
        t.backward(density_stats=True)
        assert _code(lambda: t.relocate(5, 1.0)) == 1
    with trainer("96x80") as t:                                                      # a context with a held set
        masks = torch.ones(t.n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        t.halo_commit(masks.data_ptr(), 0, 1)
        t.forward()
        t.backward(density_stats=True)
        assert _code(lambda: t.relocate(5, 1.0)) == 1
        t.synchronize()


# ---------------------------------------------------------------------------------------------
# 5. relocation
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_weight", ["inf", "median"])
def test_relocate_writes_the_planners_rows_and_invalidates_what_depends_on_them(min_weight):
    """96x80, 3 statistics steps, relocate(max_moves=20, ...).  min_weight = infinity is the case as the issue states it:
    under rules 2-3 of the planner every splat is then starved, none is a donor, and nothing moves -- which is checked, but
    proves little about the write-back; "median" (the median weight per pass, so that half of the splats are starved and
    20 pairs move) is what exercises it."""
    tgt, _ = scene("96x80")
    with trainer("96x80") as t:
        t.step(3, density_stats=True)
        stats, passes = t.density()
        assert passes == 3
        before_s = t.get_splats().view(np.float32).reshape(-1, 9).copy()
        before_a, b1, b2, it = t.get_adam()
        before_a = before_a.view(np.float32).reshape(-1, 18).copy()
        assert before_a.any()
        mw = float("inf") if min_weight == "inf" else float(np.median(stats[:, 2].astype(np.float64) / 3.0))
        ids, want_s, want_a = DP.plan(stats, passes, 20, mw, 1.6, 96, 80, before_s, before_a)
        moved = t.relocate(20, mw)
        assert moved == len(ids) == (0 if min_weight == "inf" else 20)
        got_s = t.get_splats().view(np.float32).reshape(-1, 9)
        got_a, b1n, b2n, itn = t.get_adam()
        got_a = got_a.view(np.float32).reshape(-1, 18)
        assert got_s.tobytes() == want_s.tobytes() and got_a.tobytes() == want_a.tobytes()
        others = np.setdiff1d(np.arange(t.n), ids.ravel())
        assert got_s[others].tobytes() == before_s[others].tobytes() and got_a[others].tobytes() == before_a[others].tobytes()
        if len(ids):
            assert (got_s[ids.ravel()] != before_s[ids.ravel()]).any() and not got_a[ids.ravel()].any()
        assert (b1n, b2n, itn) == (b1, b2, it)
        assert t.density()[1] == 0 and not t.density()[0].any()
        t.forward()          # lists and projection of the rows that moved must be new: the forward pass is bitwise deterministic
        img = t.get_image()
        with S2D.Trainer(96, 80, t.n) as fresh:
            fresh.set_target(tgt)
            fresh.set_splats(got_s.copy().view(S2D.SPLAT_DTYPE).reshape(-1))
            fresh.forward()
            assert img.tobytes() == fresh.get_image().tobytes()
        mse = t.step(50)
        assert np.isfinite(mse).all() and np.isfinite(t.get_splats().view(np.float32)).all()


# ---------------------------------------------------------------------------------------------
# 6. the operator and the host tool
# ---------------------------------------------------------------------------------------------
def test_operator_gathers_the_statistics_in_its_backward_call():
    import torch
    op = importlib.import_module("2dgaussiansplatting_amd.torch_op")
    tgt, splats = scene("96x80")
    up, want_abs = oracle_upstream("96x80")
    ref = oracle_stats("96x80")
    with torch.cuda.stream(torch.cuda.Stream()):
        with op.SplatRenderer(96, 80, len(splats)) as r:
            p = torch.from_numpy(splats.view(np.float32).reshape(-1, 9).copy()).cuda().requires_grad_(True)
            u = torch.from_numpy(np.ascontiguousarray(up)).cuda()
            r.render(p).backward(u)                         # without the flag: nothing gathered
            assert r.density()[1] == 0
            p.grad = None
            r.render(p, density_stats=True).backward(u)
            d, passes = r.density()
            assert passes == 1 and tuple(d.shape) == (len(splats), 3) and d.dtype == torch.float32
            stats = d.cpu().numpy()
    check_against_oracle("96x80 / operator", stats, want_abs, ref["weight"])


def test_host_tool_trains_with_relocation():
    """splat2d_train --relocate-every: status 0 and a finite trace; the final PSNR beside a plain run's is printed, not
    asserted (nobody knows yet which is higher: the defaults are provisional)."""
    train = S2D._build.build_host_program()
    base = [train, "--image", MINI, "--splats", "1024", "--iters", "300"]
    out = {}
    for name, extra in (("plain", []), ("relocate", ["--relocate-every", "100"])):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        mse = [float(m) for m in re.findall(r"^\d+ itr, mse ([-+0-9.eE]+|nan|inf)$", r.stdout, flags=re.M)]
        assert len(mse) == 300 and np.isfinite(mse).all()
        out[name] = (mse, r.stderr)
    assert out["plain"][1].count("relocated") == 0
    moved = [int(v) for v in re.findall(r"relocated (\d+) splats before iteration", out["relocate"][1])]
    assert len(moved) == 2                                   # before iterations 100 and 200
    psnr = {k: 10.0 * math.log10(255.0 ** 2 / v[0][-1]) for k, v in out.items()}
    print("\n[density] splat2d_train mini / 1024 splats / 300 iterations: final PSNR %.3f dB plain, %.3f dB with "
          "--relocate-every 100 (moved %s)" % (psnr["plain"], psnr["relocate"], moved))
