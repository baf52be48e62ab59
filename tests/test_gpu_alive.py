"""GPU tests of the alive set (include/splat2d.h, "the alive set"): s2d_set_alive, s2d_prune, s2d_grow.

The expected side of every equivalence test is the ORACLE on the alive rows compacted in index order -- OracleTrainer(target,
count) with splats[alive] -- under the bars the existing tests hold the full scene to, none of them written for this feature:
  * the framebuffer: bit-identical;
  * gradients: the three bars of oracle_lib.grad_bars; rows of dead splats all +0 bytes;
  * one step from identical state: oracle_lib.step_delta_error <= STEP_REL (tests/test_gpu_parity.py), the MSE within its
    one-step trace rtol of 2e-5; the 27 floats of a dead row byte-identical;
  * density statistics: BAR_ABS / BAR_WEIGHT of tests/test_gpu_density.py; dead rows exactly 0;
  * s2d_prune against alive_ref.prune, s2d_grow against alive_ref.lowest_dead and seed_ref.rows, s2d_relocate / s2d_reseed
    against the CPU planners on NaN-masked statistics.
Scenes: the generator of tests/test_gpu_density.py::scene with its shapes, plus 96x80 / 777 and 96x80 with n in {1, 255, 256,
257}: the 256-thread blocks of the scan and of the Adam launch.
"""
import functools
import importlib
import math
import os
import re
import subprocess

import numpy as np
import pytest

import alive_ref as AR
import loss_ref as LR
import optim_ref as OR
import oracle_lib as O
import seed_ref as SR
import test_density_plan_cpu as DP
import test_gpu_density as DN
import test_image_grads_cpu as IG
from test_gpu_parity import STEP_REL

pytestmark = pytest.mark.gpu

S2D = importlib.import_module("2dgaussiansplatting_amd")
F32 = np.float32
CHUNK = 60                           # S2D_CHUNK_PAIRS of the index-range case
TRACE_RTOL = 2e-5                    # np.testing.assert_allclose(trace, want, rtol=2e-5) of tests/test_gpu_parity.py
MINI = DN.MINI

# this file's scenes: the three shapes of test_gpu_density (its own cached arrays), and the same generator -- the same draws in
# the same order from default_rng(seed) -- on this file's additional parameters (W, H, n, seed)
EXTRA_SCENES = {"96x80_777": (96, 80, 777, 14), "96x80_n1": (96, 80, 1, 21), "96x80_n255": (96, 80, 255, 22),
                "96x80_n256": (96, 80, 256, 23), "96x80_n257": (96, 80, 257, 24)}
SCENE_PARAMS = dict(DN.RANDOM_SCENES, **EXTRA_SCENES)


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> (target, splats), as test_gpu_density.scene makes them."""
    if name not in EXTRA_SCENES:
        return DN.scene(name)
    W, H, n, seed = EXTRA_SCENES[name]
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


def trainer(name, **kw):
    tgt, splats = scene(name)
    t = S2D.Trainer(tgt.shape[1], tgt.shape[0], len(splats), **kw)
    t.set_target(tgt)
    t.set_splats(splats.view(S2D.SPLAT_DTYPE))
    return t


BASE_SCENES = ["33x17", "96x80", "40x1", "96x80_777"]
BLOCK_SCENES = ["96x80_n1", "96x80_n255", "96x80_n256", "96x80_n257"]
MASK_NAMES = ["all", "none", "one", "every_second", "first_block_dead", "last_20", "random_half"]


def n_of(name):
    return SCENE_PARAMS[name][2]


def mask_of(name, mask_name):
    return AR.masks(n_of(name), SCENE_PARAMS[name][3])[mask_name]


def cases(scenes, mask_names=MASK_NAMES):
    return [(s, m) for s in scenes for m in mask_names if m in AR.masks(n_of(s))]


ALL_CASES = cases(BASE_SCENES + BLOCK_SCENES)
PARTIAL = ["one", "every_second", "first_block_dead", "last_20", "random_half"]
GRAD_CASES = cases(BASE_SCENES, PARTIAL + ["all"]) + cases(BLOCK_SCENES, ["every_second"])


def f9(a):
    return np.ascontiguousarray(a).view(F32).reshape(-1, 9)


def f18(a):
    return np.ascontiguousarray(a).view(F32).reshape(-1, 18)


def state(t):
    a, b1, b2, it = t.get_adam()
    return f9(t.get_splats()).copy(), f18(a).copy(), (b1, b2, it)


def empty_image(H, W):
    img = np.zeros((H, W, 4), dtype=F32)
    img[..., 3] = 1.0
    return img


def compact_trainer_oracle(name, alive, fp16=False):
    tgt, splats = scene(name)
    o = O.OracleTrainer(DN._fp16(tgt) if fp16 else tgt, int(alive.sum()))
    o.splats[:] = splats[alive]
    return o


@functools.lru_cache(maxsize=None)
def compact_oracle(name, mask_name, fp16=False):
    """The oracle on the alive rows of a scene, computed once: image, gradient sums (w32, dsum, dabs), density weight, and
    the state and MSE after one step."""
    tgt, splats = scene(name)
    alive = mask_of(name, mask_name)
    r = {"alive": alive, "count": int(alive.sum())}
    if r["count"] == 0:
        r["image"] = empty_image(*tgt.shape[:2])
        return r
    o = compact_trainer_oracle(name, alive, fp16)
    o.forward()
    if fp16:
        o.image0[:] = DN._fp16(o.image0)
    r["image"] = o.image0.copy()
    d, dsum, dabs = o.backward_stats()
    r["w32"], r["dsum"], r["dabs"] = f9(d).copy(), dsum.copy(), dabs.copy()
    r["weight"] = DN._weight_from(o)
    if not fp16:
        s = compact_trainer_oracle(name, alive)
        st, mse = s.step()
        assert st == 0
        r["after_s"], r["after_a"], r["mse"] = f9(s.splats).copy(), f18(s.adams).copy(), mse
    return r


@functools.lru_cache(maxsize=None)
def full_image(name):
    tgt, splats = scene(name)
    o = O.OracleTrainer(tgt, len(splats))
    o.splats[:] = splats
    return o.forward().copy()


def masked_trainer(name, mask_name, **kw):
    t = trainer(name, **kw)
    t.set_alive(mask_of(name, mask_name))
    return t


def assert_dead_rows_untouched(label, alive, before, after):
    (s0, a0, _), (s1, a1, _) = before, after
    assert s1[~alive].tobytes() == s0[~alive].tobytes(), label
    assert a1[~alive].tobytes() == a0[~alive].tobytes(), label


# ---------------------------------------------------------------------------------------------
# 1. forward
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mask_name", ALL_CASES)
def test_forward_equals_the_compacted_oracle(name, mask_name):
    ref = compact_oracle(name, mask_name)
    with masked_trainer(name, mask_name) as t:
        t.forward()
        img = t.get_image()
        got_alive, count = t.alive()
    assert img.tobytes() == ref["image"].tobytes()
    assert got_alive.tolist() == ref["alive"].tolist() and count == ref["count"]
    if mask_name == "none":
        assert not img[..., :3].any() and (img[..., 3] == 1).all()


@pytest.mark.parametrize("variant", ["fp16_images", "generic_binning", "index_ranges", "count_pairs", "exact_exp_runs"])
@pytest.mark.parametrize("mask_name", ["every_second", "first_block_dead", "random_half"])
def test_forward_of_the_other_context_kinds(variant, mask_name):
    name = "96x80"
    fp16 = variant == "fp16_images"
    ref = compact_oracle(name, mask_name, fp16)
    kw = {"fp16_images": {"fp16_images": True}, "generic_binning": {"generic_binning": True}, "index_ranges": {"chunk_pairs": CHUNK},
          "count_pairs": {"count_pairs": True}, "exact_exp_runs": {"exact_exp": True}}[variant]
    with masked_trainer(name, mask_name, **kw) as t:
        t.forward()
        img = t.get_image()
        if variant == "index_ranges":          # a budget small enough to cut the alive rows of 96x80 / 300 into >= 3 ranges:
            total = sum_pairs_of(name, mask_name)              # no range holds more than the budget (a splat has < CHUNK pairs here)
            assert total > 2 * CHUNK and t.stats()["pairs_binned"] <= CHUNK, (total, t.stats()["pairs_binned"])
        t.backward()
        assert not f9(t.get_grads())[~ref["alive"]].view(np.uint32).any()
    if variant == "exact_exp_runs":            # expf instead of the reference's approximation: the compact context of that kind
        tgt, splats = scene(name)
        with S2D.Trainer(96, 80, ref["count"], exact_exp=True) as c:
            c.set_target(tgt)
            c.set_splats(np.ascontiguousarray(splats[ref["alive"]]).view(S2D.SPLAT_DTYPE))
            c.forward()
            assert img.tobytes() == c.get_image().tobytes()
    else:
        assert img.tobytes() == ref["image"].tobytes()


@functools.lru_cache(maxsize=None)
def sum_pairs_of(name, mask_name):
    """(tile, splat) pairs of the alive rows' lists in one set (a context without a chunk limit)."""
    with masked_trainer(name, mask_name) as t:
        t.forward()
        return int(t.stats()["pairs_binned"])


# ---------------------------------------------------------------------------------------------
# 2. gradients
# ---------------------------------------------------------------------------------------------
def check_grads(label, got9, ref, skip_opacity):
    alive = ref["alive"]
    assert not got9[~alive].view(np.uint32).any(), label + ": a dead row's gradient record is not +0 bytes"
    w32, dsum, dabs = ref["w32"].copy(), ref["dsum"].copy(), ref["dabs"].copy()
    if skip_opacity:                           # the column is left at zero: held to exactly that
        w32[:, 8], dsum[:, 8], dabs[:, 8] = 0, 0, 0
    bars = O.grad_bars(got9[alive], w32, dsum, dabs)
    print("\n[alive] %s: (a) %.3e (b) %.3e (c) %.3e" % (label, bars["a_gpu_vs_exact"], bars["b_ref_vs_exact"], bars["c_gpu_vs_oracle"]))


@pytest.mark.parametrize("name,mask_name", GRAD_CASES)
def test_gradients_match_the_compacted_oracle(name, mask_name):
    ref = compact_oracle(name, mask_name)
    for det in (False, True):
        for skip in (False, True):
            with masked_trainer(name, mask_name, deterministic=det) as t:
                t.forward()
                t.backward(skip_opacity_grad=skip)
                check_grads("%s / %s / det=%s skip=%s backward" % (name, mask_name, det, skip), f9(t.get_grads()), ref, skip)
                mse_b = t.mse()
            with masked_trainer(name, mask_name, deterministic=det) as t:
                t.forward_backward(skip_opacity_grad=skip)
                check_grads("%s / %s / det=%s skip=%s forward_backward" % (name, mask_name, det, skip), f9(t.get_grads()), ref, skip)
                assert t.get_image().tobytes() == ref["image"].tobytes() and t.mse() == mse_b


@pytest.mark.parametrize("name", BASE_SCENES + BLOCK_SCENES)
def test_no_row_alive_leaves_every_gradient_record_at_plus_zero(name):
    for det in (False, True):
        with masked_trainer(name, "none", deterministic=det) as t:
            t.forward()
            t.backward()
            assert not f9(t.get_grads()).view(np.uint32).any()
            t.forward_backward()
            assert not f9(t.get_grads()).view(np.uint32).any()
            assert t.get_image().tobytes() == compact_oracle(name, "none")["image"].tobytes()


@functools.lru_cache(maxsize=None)
def compact_upstream(name, mask_name):
    """The signed, masked upstream of test_image_grads_cpu on the compacted scene: (upstream, w32, dsum, dabs)."""
    tgt, _ = scene(name)
    o = compact_trainer_oracle(name, mask_of(name, mask_name))
    img = o.forward().copy()
    g = IG.charbonnier_grad(img, tgt, IG.charbonnier_weights(*tgt.shape[:2]))
    pseudo = IG.pseudo_target(img, g)
    o.ref = np.ascontiguousarray(pseudo)
    d, dsum, dabs = o.backward_stats()
    up = IG.upstream_of(img, pseudo)
    assert (up[..., :3] < 0).any() and (up[..., :3] > 0).any()
    return up, f9(d).copy(), dsum.copy(), dabs.copy()


@pytest.mark.parametrize("det", [False, True], ids=["atomic", "deterministic"])
@pytest.mark.parametrize("name,mask_name", cases(["96x80", "96x80_777"], ["every_second", "first_block_dead", "random_half"]))
def test_image_grads_entry_point_with_a_mask(name, mask_name, det):
    import torch
    up, w32, dsum, dabs = compact_upstream(name, mask_name)
    alive = mask_of(name, mask_name)
    with masked_trainer(name, mask_name, deterministic=det) as t:
        t.forward()
        u = torch.from_numpy(np.ascontiguousarray(up)).cuda()
        torch.cuda.synchronize()
        t.backward_image_grads(u.data_ptr(), skip_opacity_grad=False)
        got = f9(t.get_grads())
    check_grads("%s / %s / upstream det=%s" % (name, mask_name, det), got, {"alive": alive, "w32": w32, "dsum": dsum, "dabs": dabs}, False)


# ---------------------------------------------------------------------------------------------
# 3. one step from identical state
# ---------------------------------------------------------------------------------------------
def check_step(label, alive, before, after, want_s, lr=0.05):
    err = O.step_delta_error(before[0][alive], after[0][alive], want_s, lr=lr)
    print("\n[alive] %s: step delta error %.3e of lr (bar %.1e)" % (label, float(err.max()) if err.size else 0.0, STEP_REL))
    assert err.size == 0 or err.max() <= STEP_REL, err.max()
    assert_dead_rows_untouched(label, alive, before, after)
    assert after[2][2] == before[2][2] + 1


STEP_CASES = cases(BASE_SCENES, PARTIAL) + cases(BLOCK_SCENES, ["all", "one", "every_second"])


@pytest.mark.parametrize("path", ["fused", "density_stats"])
@pytest.mark.parametrize("name,mask_name", STEP_CASES)
def test_one_step_matches_the_compacted_oracle(name, mask_name, path):
    ref = compact_oracle(name, mask_name)
    alive = ref["alive"]
    with masked_trainer(name, mask_name) as t:
        before = state(t)
        mse = t.step(1, density_stats=(path == "density_stats"))
        after = state(t)
        stats, passes = t.density()
    check_step("%s / %s / %s" % (name, mask_name, path), alive, before, after, ref["after_s"])
    assert abs(mse[0] - ref["mse"]) <= TRACE_RTOL * ref["mse"], (mse[0], ref["mse"])
    if path == "density_stats":
        assert passes == 1 and not stats[~alive].view(np.uint32).any()
    else:
        assert passes == 0


def test_no_row_alive_steps_nothing():
    name = "96x80"
    with masked_trainer(name, "none") as t:
        before = state(t)
        mse = t.step(3)
        after = state(t)
        assert t.get_image().tobytes() == empty_image(80, 96).tobytes()
    assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
    tgt, _ = scene(name)
    o = O.OracleTrainer(tgt, 1)
    o.image0[:] = empty_image(80, 96)
    assert np.all(np.abs(mse - o.mse()) <= 1e-9 * o.mse()) and after[2][2] == 3


@pytest.mark.parametrize("name,mask_name", cases(["96x80", "96x80_777"], ["every_second", "first_block_dead", "random_half"]))
def test_one_loss_step_matches_the_oracle_under_the_losses_gradient(name, mask_name):
    """step_loss with weights (0, 0.8, 0.2): the expected step is the oracle's on the compacted rows under the pseudo-target of
    dL/d(image0), formed in float64 by loss_ref.torch_loss on the framebuffer (which is the oracle's, bit for bit)."""
    tgt, _ = scene(name)
    alive = mask_of(name, mask_name)
    o = compact_trainer_oracle(name, alive)
    img = o.forward().copy()
    g = np.zeros_like(img)
    g[..., :3] = LR.torch_loss(img, tgt, (0.0, 0.8, 0.2))["grad"].astype(F32)
    o.ref = np.ascontiguousarray(IG.pseudo_target(img, g))
    o.backward()
    assert o.adam() == 0
    with masked_trainer(name, mask_name) as t:
        before = state(t)
        loss, mse = t.step_loss(1, 0.0, 0.8, 0.2)
        after = state(t)
    check_step("%s / %s / step_loss" % (name, mask_name), alive, before, after, f9(o.splats))
    assert np.isfinite(loss).all() and abs(mse[0] - compact_oracle(name, mask_name)["mse"]) <= TRACE_RTOL * mse[0]


@pytest.mark.parametrize("name,mask_name", cases(["96x80", "96x80_777"], ["every_second", "first_block_dead", "random_half"]))
def test_one_step_under_group_rates_and_a_frozen_mask(name, mask_name):
    """set_optim + a frozen mask that overlaps the alive set: the composite oracle of tests/optim_ref.py on the compacted rows.
    A row trains only when it is alive and not frozen; frozen and alive rows are byte-identical, like the dead ones."""
    ref = compact_oracle(name, mask_name)
    alive = ref["alive"]
    n = len(alive)
    frozen = np.random.default_rng(77).random(n) < 0.4
    assert (frozen & alive).any() and (frozen & ~alive).any() and (~frozen & alive).any()
    tgt, splats = scene(name)
    k = ref["count"]
    want_s = f9(splats[alive]).copy()
    want_a = np.zeros((k, 9, 2), dtype=F32)
    rates = np.array(OR.GAIN_RATES, dtype=F32)
    b1, b2 = np.ones(1, dtype=F32), np.ones(1, dtype=F32)
    assert OR.composite_step(want_s, want_a, ref["w32"], 96, 80, b1, b2, False, rates, frozen[alive]) == 0
    with masked_trainer(name, mask_name) as t:
        t.set_optim(*[float(r) for r in rates])
        t.set_frozen(frozen)
        before = state(t)
        t.step(1)
        after = state(t)
        assert t.alive()[0].tolist() == alive.tolist()            # s2d_set_optim / s2d_set_frozen keep the set
    lr9 = np.array([rates[g] for g in OR.GROUP_OF], dtype=np.float64)
    check_step("%s / %s / controls" % (name, mask_name), alive, before, after, want_s, lr=lr9)
    still = frozen & alive
    assert after[0][still].tobytes() == before[0][still].tobytes() and after[1][still].tobytes() == before[1][still].tobytes()
    moved = alive & ~frozen
    assert (after[0][moved] != before[0][moved]).any()


# ---------------------------------------------------------------------------------------------
# 4. / 5. GPU against GPU, deterministic
# ---------------------------------------------------------------------------------------------
def five_steps(t):
    mse = t.step(5)
    s, a, it = state(t)
    return mse.tobytes(), s, a, it


@pytest.mark.parametrize("name,mask_name", cases(["96x80", "96x80_777", "96x80_n257"], ["every_second", "first_block_dead", "random_half", "last_20"]))
def test_five_deterministic_steps_equal_the_compact_context_bytewise(name, mask_name):
    """Each splat's tiles, per-tile partial sums and gather order depend on its rectangle, not on its index: a context with
    a mask and a fresh context of n_splats = count holding the compacted rows are expected bytes-equal."""
    tgt, splats = scene(name)
    alive = mask_of(name, mask_name)
    with masked_trainer(name, mask_name, deterministic=True) as t:
        before = state(t)
        mse_m, s_m, a_m, it_m = five_steps(t)
    with S2D.Trainer(96, 80, int(alive.sum()), deterministic=True) as c:
        c.set_target(tgt)
        c.set_splats(np.ascontiguousarray(splats[alive]).view(S2D.SPLAT_DTYPE))
        mse_c, s_c, a_c, it_c = five_steps(c)
    assert mse_m == mse_c and it_m == it_c
    assert s_m[alive].tobytes() == s_c.tobytes() and a_m[alive].tobytes() == a_c.tobytes()
    assert s_m[~alive].tobytes() == before[0][~alive].tobytes() and not a_m[~alive].any()
    assert (s_m[alive] != before[0][alive]).any()


def test_an_all_ones_set_and_a_cleared_set_equal_no_set():
    name = "96x80_777"
    tgt, splats = scene(name)
    with trainer(name, deterministic=True) as plain:
        want = five_steps(plain)
    with masked_trainer(name, "all", deterministic=True) as t:
        got = five_steps(t)
        assert t.alive()[1] == 777
    assert got[0] == want[0] and got[1].tobytes() == want[1].tobytes() and got[2].tobytes() == want[2].tobytes() and got[3] == want[3]
    # set_alive(None) after a mask and some steps, followed by a step, equals a fresh context given the same state
    with masked_trainer(name, "random_half", deterministic=True) as t:
        t.step(2)
        t.set_alive(None)
        assert t.alive()[0].all() and t.alive()[1] == 777
        s, a, (b1, b2, it) = state(t)
        got = five_steps(t)
    with S2D.Trainer(96, 80, 777, deterministic=True) as fresh:
        fresh.set_target(tgt)
        fresh.set_splats(s.copy().view(S2D.SPLAT_DTYPE).reshape(-1))
        fresh.set_adam(a.copy().view(S2D.ADAM_DTYPE).reshape(-1), b1, b2, it)
        want = five_steps(fresh)
    assert got[0] == want[0] and got[1].tobytes() == want[1].tobytes() and got[2].tobytes() == want[2].tobytes() and got[3] == want[3]


# ---------------------------------------------------------------------------------------------
# 6. density statistics with a mask
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["default", "deterministic", "fp16_images"])
@pytest.mark.parametrize("name,mask_name", cases(["33x17", "96x80", "96x80_777"], ["every_second", "first_block_dead", "random_half"]))
def test_density_statistics_with_a_mask(name, mask_name, variant):
    kw = DN.VARIANTS[variant][0]
    ref = compact_oracle(name, mask_name, bool(kw.get("fp16_images")))
    alive = ref["alive"]
    with masked_trainer(name, mask_name, **kw) as t:
        t.forward()
        t.backward(density_stats=True)
        stats, passes = t.density()
    assert passes == 1 and not stats[~alive].view(np.uint32).any()
    DN.check_against_oracle("%s / %s / %s with a mask" % (name, mask_name, variant), stats[alive], ref["dabs"][:, 0:2], ref["weight"])


# ---------------------------------------------------------------------------------------------
# 7. set_alive invalidates
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [{}, {"deterministic": True}], ids=["atomic", "deterministic"])
def test_set_alive_invalidates_the_lists_in_both_directions(kw):
    name = "96x80"
    with trainer(name, **kw) as t:
        t.step(1)                                              # lists, projection and a fused Adam projection exist
        tgt, _ = scene(name)
        s = f9(t.get_splats()).copy()

        def oracle_image(alive):
            o = O.OracleTrainer(tgt, int(alive.sum()))
            o.splats[:] = s[alive].copy().view(O.SPLAT_DTYPE).reshape(-1)
            return o.forward().copy()

        t.forward()
        assert t.get_image().tobytes() == oracle_image(np.ones(300, dtype=bool)).tobytes()
        builds = t.rebuild_count()
        alive = mask_of(name, "random_half")
        t.set_alive(alive)                                     # departures only: their list entries must not be drawn
        t.forward()
        assert t.get_image().tobytes() == oracle_image(alive).tobytes()
        assert t.rebuild_count() == builds + 1
        got, count = t.alive()
        assert got.dtype == bool and got.tolist() == alive.tolist() and count == int(alive.sum())
        raw = np.full(300, 7, dtype=np.uint8)
        assert t.L.s2d_get_alive(t._h, raw.ctypes.data, None) == 0 and set(raw.tolist()) == {0, 1}
        t.set_alive(np.where(alive, 200, 0).astype(np.uint8))  # any non-zero byte is alive; the same set again
        assert t.alive()[0].tolist() == alive.tolist()
        builds = t.rebuild_count()
        t.set_alive(np.ones(300, dtype=bool))                  # arrivals
        t.forward()
        assert t.get_image().tobytes() == oracle_image(np.ones(300, dtype=bool)).tobytes()
        assert t.rebuild_count() == builds + 1
        t.set_alive(alive)
        t.set_splats(s.copy().view(S2D.SPLAT_DTYPE).reshape(-1))      # s2d_set_splats keeps the set
        assert t.alive()[1] == int(alive.sum())
        t.init()                                               # s2d_init_splats clears it
        assert t.alive()[0].all() and t.alive()[1] == 300
        t.forward()
        o = O.OracleTrainer(tgt, 300)
        assert t.get_image().tobytes() == o.forward().tobytes()


def test_set_alive_from_device_memory():
    import torch
    name = "96x80_777"
    ref = compact_oracle(name, "random_half")
    with trainer(name) as t:
        m = torch.from_numpy(ref["alive"].astype(np.uint8) * 3).cuda()
        torch.cuda.synchronize()
        t.set_alive_device(m.data_ptr())
        t.forward()
        assert t.get_image().tobytes() == ref["image"].tobytes()
        assert t.alive()[0].tolist() == ref["alive"].tolist() and t.alive()[1] == ref["count"]
        t.set_alive_device(None)
        assert t.alive()[1] == 777
        t.forward()
        assert t.get_image().tobytes() == full_image(name).tobytes()


# ---------------------------------------------------------------------------------------------
# 8. prune
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("criterion", ["weight", "opacity", "both"])
@pytest.mark.parametrize("name", ["96x80", "96x80_777"])
def test_prune_follows_the_rule(name, criterion):
    tgt, _ = scene(name)
    with trainer(name) as t:
        n = t.n
        t.step(3, density_stats=True)
        stats, passes = t.density()
        before = state(t)
        alive0, count0 = t.alive()
        assert passes == 3 and count0 == n and alive0.all()
        mw = float(F32(np.median(stats[:, 2].astype(np.float64) / 3.0))) if criterion in ("weight", "both") else 0.0
        mo = 0.5 if criterion in ("opacity", "both") else 0.0
        want = AR.prune(alive0, stats, passes, before[0][:, 8], mw, mo)
        share = 1.0 - want.sum() / n
        print("\n[alive] prune %s / %s: min_weight %.6g min_opacity %.2f prunes %.1f %% of %d" % (name, criterion, mw, mo, 100 * share, n))
        assert 0.10 <= share <= 0.90                           # the premise, on this project's own statistics
        pruned = t.prune(min_weight=mw, min_opacity=mo)
        got, count = t.alive()
        assert got.tolist() == want.tolist() and pruned == n - int(want.sum()) and count == int(want.sum())
        after = state(t)
        assert after[0].tobytes() == before[0].tobytes() and after[1].tobytes() == before[1].tobytes() and after[2] == before[2]
        if mw > 0:
            assert t.density()[1] == 0 and not t.density()[0].any()
        else:
            assert t.density()[1] == 3 and t.density()[0].tobytes() == stats.tobytes()
        t.forward()
        o = O.OracleTrainer(tgt, int(want.sum()))
        o.splats[:] = before[0][want].copy().view(O.SPLAT_DTYPE).reshape(-1)
        assert t.get_image().tobytes() == o.forward().tobytes()
        if mo > 0:                                             # the same statistics-free criterion again prunes nothing
            builds = t.rebuild_count()
            assert t.prune(min_opacity=mo) == 0 and t.alive()[0].tolist() == want.tolist()
            t.forward()
            assert t.rebuild_count() == builds
        # a second round starts from the set: dead rows stay dead whatever their values
        t.step(2, density_stats=True)
        stats2, passes2 = t.density()
        s2 = f9(t.get_splats())
        want2 = AR.prune(want, stats2, passes2, s2[:, 8], mw if mw > 0 else 0.0, 0.3)
        t.prune(min_weight=mw if mw > 0 else 0.0, min_opacity=0.3)
        assert t.alive()[0].tolist() == want2.tolist() and not (want2 & ~want).any()


# ---------------------------------------------------------------------------------------------
# 9. grow
# ---------------------------------------------------------------------------------------------
def last_alive(n, k):
    m = np.zeros(n, dtype=bool)
    m[n - k:] = True
    return m


def seed_rows_of(t, ids, tgt, image0, source, seed, scale):
    q, total = SR.importance({"error": SR.ERROR, "edges": SR.EDGES}[source], ref=tgt, image0=image0, squared=True)
    return SR.rows(ids, seed, q, total, tgt, t.n, scale=scale), total


@pytest.mark.parametrize("explicit", [False, True], ids=["lowest_dead", "explicit_ids"])
def test_grow_seeds_the_chosen_rows_and_brings_them_to_life(explicit):
    name = "96x80"
    tgt, splats = scene(name)
    alive = last_alive(300, 50)
    with trainer(name) as t:
        t.set_alive(alive)
        t.step(2)                                              # moments of the alive rows are no longer zero
        t.forward()
        image0 = t.get_image()
        before = state(t)
        q_gpu, total_gpu = t.importance(source="error", squared=True)
        if explicit:
            ids = np.array([17, 3, 240, 99, 100], dtype=np.int32)
            for bad in ([17, 17], [3, 299], [300], [-1]):      # repeated, alive, out of range
                with pytest.raises(S2D.S2DError) as e:
                    t.grow(0, ids=bad, source="error", squared=True, seed=5, scale=2.5)
                assert e.value.code == 1
                assert t.alive()[0].tolist() == alive.tolist() and state(t)[0].tobytes() == before[0].tobytes()
            grown = t.grow(0, ids=ids, source="error", squared=True, seed=5, scale=2.5)
        else:
            ids = AR.lowest_dead(alive, 40)
            assert ids.tolist() == list(range(40))
            grown = t.grow(40, source="error", squared=True, seed=5, scale=2.5)
        assert grown == len(ids)
        want_rows, total = seed_rows_of(t, ids, tgt, image0, "error", 5, 2.5)
        assert total == total_gpu and total > 0
        after = state(t)
        assert after[0][ids].tobytes() == want_rows.tobytes() and not after[1][ids].view(np.uint32).any()
        others = np.setdiff1d(np.arange(300), ids)
        assert after[0][others].tobytes() == before[0][others].tobytes() and after[1][others].tobytes() == before[1][others].tobytes()
        assert after[2] == before[2]
        want_alive = alive.copy()
        want_alive[ids] = True
        got, count = t.alive()
        assert got.tolist() == want_alive.tolist() and count == 50 + len(ids)
        t.forward()
        o = O.OracleTrainer(tgt, count)
        o.splats[:] = after[0][want_alive].copy().view(O.SPLAT_DTYPE).reshape(-1)
        assert t.get_image().tobytes() == o.forward().tobytes()
        if not explicit:
            t.forward()
            assert t.grow(10 ** 6, source="error", squared=True, seed=6) == 300 - 90      # what is left
            assert t.alive()[0].all() and t.alive()[1] == 300
            t.forward()
            assert t.grow(5, source="error", squared=True, seed=7) == 0
            s = f9(t.get_splats())
            t.forward()
            full = O.OracleTrainer(tgt, 300)
            full.splats[:] = s.copy().view(O.SPLAT_DTYPE).reshape(-1)
            assert t.get_image().tobytes() == full.forward().tobytes()
            mse = t.step(3)
            assert np.isfinite(mse).all()


def test_grow_state_rules_and_an_empty_map():
    name = "96x80"
    alive = last_alive(300, 50)
    with trainer(name) as t:
        t.set_alive(alive)
        before = state(t)
        with pytest.raises(S2D.S2DError) as e:                 # the error map needs a forward pass on the current parameters
            t.grow(10, source="error")
        assert e.value.code == 5 and t.alive()[0].tolist() == alive.tolist()
        assert t.grow(0, source="edges") == 0 and t.alive()[1] == 50
        assert t.grow(10, source="edges", seed=3) == 10        # the edge map needs none
        assert t.alive()[1] == 60 and t.alive()[0][:10].all()
    with trainer(name) as t:                                # a black target has no edges: total 0, nothing changes
        t.set_target(empty_image(80, 96))
        t.set_alive(alive)
        builds = t.rebuild_count()
        t.forward()
        assert t.importance(source="edges")[1] == 0
        assert t.grow(10, source="edges") == 0
        assert t.alive()[0].tolist() == alive.tolist() and state(t)[0].tobytes() == before[0].tobytes()
        t.forward()
        assert t.rebuild_count() == builds + 1                 # (the one build of the first forward)
    with trainer(name) as t:                                # without a set no row is dead
        assert t.grow(10, source="edges") == 0 and t.alive()[1] == 300


# ---------------------------------------------------------------------------------------------
# 10. relocate / reseed with a mask
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask_name", ["every_second", "random_half", "first_block_dead"])
def test_relocate_and_reseed_leave_dead_rows_alone(mask_name):
    name = "96x80_777"
    tgt, _ = scene(name)
    alive = mask_of(name, mask_name)
    for call in ("relocate", "reseed"):
        with masked_trainer(name, mask_name) as t:
            t.step(3, density_stats=True)
            stats, passes = t.density()
            assert passes == 3 and not stats[~alive].any()
            before = state(t)
            masked = AR.nan_masked(stats, alive)
            mw = float(F32(np.median(stats[alive, 2].astype(np.float64) / 3.0)))
            if call == "relocate":
                ids, want_s, want_a = DP.plan(masked, passes, 40, mw, 1.6, 96, 80, before[0], before[1])
                moved = t.relocate(40, mw)
                assert moved == len(ids) > 0
                touched = ids.ravel()
                after = state(t)
                assert after[0].tobytes() == want_s.tobytes() and after[1].tobytes() == want_a.tobytes()
            else:
                t.forward()
                image0 = t.get_image()
                touched = SR.starved(masked, passes, 40, mw)
                assert len(touched) > 0
                # (unmasked, dead rows -- weight 0 -- would be among the first to be named)
                assert (~alive[SR.starved(stats, passes, 40, mw)]).any()
                moved = t.reseed(40, mw, source="error", squared=True, seed=9, scale=2.0)
                assert moved == len(touched)
                after = state(t)
                want_rows, total = seed_rows_of(t, touched, tgt, image0, "error", 9, 2.0)
                assert total > 0 and after[0][touched].tobytes() == want_rows.tobytes()
                others = np.setdiff1d(np.arange(t.n), touched)
                assert after[0][others].tobytes() == before[0][others].tobytes()
            assert alive[touched].all(), call
            assert_dead_rows_untouched(call, alive, before, after)
            assert t.alive()[0].tolist() == alive.tolist()
            t.forward()
            o = O.OracleTrainer(tgt, int(alive.sum()))
            o.splats[:] = after[0][alive].copy().view(O.SPLAT_DTYPE).reshape(-1)
            assert t.get_image().tobytes() == o.forward().tobytes()


# ---------------------------------------------------------------------------------------------
# 11. status codes
# ---------------------------------------------------------------------------------------------
def _code(call):
    with pytest.raises(S2D.S2DError) as e:
        call()
    return e.value.code


def all_alive_calls(t):
    m = np.ones(t.n, dtype=bool)
    return [lambda: t.set_alive(m), lambda: t.set_alive(None), lambda: t.set_alive_device(None), lambda: t.alive(),
            lambda: t.prune(min_opacity=0.5), lambda: t.grow(5, source="edges")]


def test_status_codes():
    import torch
    name = "96x80"
    alive = mask_of(name, "random_half")
    with masked_trainer(name, "random_half") as t:
        t.forward()
        img = t.get_image().tobytes()
        for bad in (lambda: t.prune(), lambda: t.prune(min_weight=-1.0), lambda: t.prune(min_opacity=-0.5),
                    lambda: t.prune(min_weight=float("nan")), lambda: t.prune(min_opacity=float("nan"))):
            assert _code(bad) == 1
        assert t.L.s2d_prune(t._h, None, None) == 1
        assert t.L.s2d_prune(t._h, S2D._PruneConfig(8, 0.0, 0.5), None) == 1
        assert _code(lambda: t.prune(min_weight=1.0)) == 5                     # no statistics pass since the last reset
        for bad in (lambda: t.grow(-1, source="edges"), lambda: t.grow(5, source="edges", floor=5000), lambda: t.grow(5, source="edges", scale=-1.0),
                    lambda: t.grow(5, source="edges", opacity=2.0), lambda: t.grow(5, source=7), lambda: t.grow(5, source="caller")):
            assert _code(bad) == 1
        masks = torch.ones(t.n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert _code(lambda: t.halo_commit(masks.data_ptr(), 0, 1)) == 1       # the two kinds of subset exclude each other
        assert _code(lambda: t.halo_masks([0, 80], 0.0, masks.data_ptr())) == 1
        builds = t.rebuild_count()
        assert t.alive()[0].tolist() == alive.tolist()                         # nothing of a refused call sticks
        t.forward()
        assert t.get_image().tobytes() == img and t.rebuild_count() == builds
        t.backward(density_stats=True)
        assert _code(lambda: t.relocate(-1, 1.0)) == 1 and t.density()[1] == 1
    with trainer(name, reference_order=True) as t:
        for call in all_alive_calls(t):
            assert _code(call) == 1
        t.forward()
    with trainer(name, row_begin=16, row_end=48) as t:                      # a slab context
        for call in all_alive_calls(t):
            assert _code(call) == 1
        t.forward()
    with trainer(name) as t:                                                # a context with a held set keeps its refusals
        masks = torch.ones(t.n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        t.halo_commit(masks.data_ptr(), 0, 1)
        for call in all_alive_calls(t):
            assert _code(call) == 1
        t.forward()
        t.backward(density_stats=True)
        assert _code(lambda: t.relocate(5, 1.0)) == 1
        assert _code(lambda: t.set_frozen(np.zeros(t.n, dtype=bool))) == 1
        assert _code(lambda: t.seed(source="edges")) == 1
        t.synchronize()


# ---------------------------------------------------------------------------------------------
# 12. the torch operator
# ---------------------------------------------------------------------------------------------
def test_operator_with_a_mask():
    import torch
    op = importlib.import_module("2dgaussiansplatting_amd.torch_op")
    name, mask_name = "96x80", "random_half"
    tgt, splats = scene(name)
    ref = compact_oracle(name, mask_name)
    alive = ref["alive"]
    up, _, _, _ = compact_upstream(name, mask_name)
    with torch.cuda.stream(torch.cuda.Stream()):
        u = torch.from_numpy(np.ascontiguousarray(up)).cuda()
        with op.SplatRenderer(96, 80, 300) as r:
            r.set_alive(alive)
            p = torch.from_numpy(f9(splats).copy()).cuda().requires_grad_(True)
            img = r.render(p)
            assert img.detach().cpu().numpy().tobytes() == ref["image"].tobytes()
            img.backward(u)
            g = p.grad.detach().cpu().numpy()
            assert r.alive()[1] == ref["count"]
        with op.SplatRenderer(96, 80, ref["count"]) as c:                      # the unmasked operator on the compacted scene
            pc = torch.from_numpy(f9(splats[alive]).copy()).cuda().requires_grad_(True)
            c.render(pc).backward(u)
            gc = pc.grad.detach().cpu().numpy()
    assert g.shape == (300, 9) and not g[~alive].view(np.uint32).any()
    _, w32, dsum, dabs = compact_upstream(name, mask_name)
    nz = dabs > 0
    c_bar = float((np.abs(g[alive].astype(np.float64) - gc)[nz] / np.maximum(np.abs(gc[nz]), 0.02 * dabs[nz])).max())
    print("\n[alive] operator with a mask against the operator on the compacted scene: bar (c) %.3e" % c_bar)
    assert c_bar <= 1e-4
    check_grads("operator with a mask", g, {"alive": alive, "w32": w32, "dsum": dsum, "dabs": dabs}, False)


# ---------------------------------------------------------------------------------------------
# 13. the host tool
# ---------------------------------------------------------------------------------------------
def test_host_tool_grows_and_prunes():
    """splat2d_train with --alive-from / --grow-every, then --prune-every: status 0, finite traces, the events it reports.  The
    final PSNR beside a plain run's is printed, not asserted (one run, a first data point: the defaults are provisional)."""
    train = S2D._build.build_host_program()
    base = [train, "--image", MINI, "--splats", "1024", "--iters", "300"]
    runs = {"plain": [], "grow": ["--alive-from", "256", "--grow-every", "50", "--grow-count", "256"],
            "grow_prune": ["--alive-from", "256", "--grow-every", "50", "--grow-count", "256", "--prune-every", "100"]}
    out = {}
    for name, extra in runs.items():
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        mse = [float(m) for m in re.findall(r"^\d+ itr, mse ([-+0-9.eE]+|nan|inf)$", r.stdout, flags=re.M)]
        assert len(mse) == 300 and np.isfinite(mse).all()
        out[name] = (mse, r.stderr)
    assert "alive" not in out["plain"][1]
    grew = [(int(a), int(b), int(c)) for a, b, c in re.findall(r"grew (\d+) splats before iteration (\d+), (\d+) alive", out["grow"][1])]
    assert grew == [(256, 50, 512), (256, 100, 768), (256, 150, 1024)]
    assert "256 of 1024 splats alive at the start" in out["grow"][1] and "1024 of 1024 splats alive at the end" in out["grow"][1]
    pruned = [(int(a), int(b), int(c)) for a, b, c in re.findall(r"pruned (\d+) splats before iteration (\d+), (\d+) alive", out["grow_prune"][1])]
    assert [p[1] for p in pruned] == [100, 200] and all(0 <= p[0] <= 1024 and 0 < p[2] <= 1024 for p in pruned)
    end = int(re.search(r"(\d+) of 1024 splats alive at the end", out["grow_prune"][1]).group(1))
    psnr = {k: 10.0 * math.log10(255.0 ** 2 / v[0][-1]) for k, v in out.items()}
    print("\n[alive] splat2d_train mini / 1024 splats / 300 iterations: final PSNR %.3f dB plain, %.3f dB grown from 256 in three "
          "steps, %.3f dB with --prune-every 100 on top (pruned %s, %d alive at the end)"
          % (psnr["plain"], psnr["grow"], psnr["grow_prune"], [p[0] for p in pruned], end))
    for extra, word in ((["--alive-from", "10", "--gpus", "2"], "one context"), (["--alive-from", "10", "--reference-order"], "--reference-order"),
                        (["--prune-every", "2", "--relocate-every", "2"], "statistics window"), (["--alive-from", "10", "--save-checkpoint", "x"], "checkpoint")):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and word in r.stderr and not r.stdout, extra
