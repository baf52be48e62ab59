"""The forward walk hands the backward walk the entries it executed, compacted (s2d_walk.h forward_tile).

A counting context (count_pairs=True) keeps the older hand-over -- every staged entry at its list position, the backward
walk going through the tile's whole list -- so the two paths are two implementations of the same sums.  With
deterministic=True every per-(tile, splat) partial is a fixed-order sum of the same per-wave sums and the gather is the
same, so everything below is compared byte for byte: image, MSE, gradients, and after training steps the parameters
and the Adam moments.  Framebuffers are also held against the oracle's, bit for bit.

The forward walk also sizes its batches by where the tile retired in the previous launch of the context (a hint that
nothing ever resets); a counting context has no such hint, so the same comparisons show that it changes nothing.
"""
import importlib
import os

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

S2D = importlib.import_module("2dgaussiansplatting_amd")
MINI = os.path.join(O.GOLDEN, "squirrel_cls_mini_268x213.s2di")
FULL = os.path.join(O.GOLDEN, "squirrel_cls_535x426.s2di")


def _target(path):
    return O.target_rgba32f(O.load_s2di(path))


def _fp16(a):
    return a.astype(np.float16).astype(np.float32)


def _random_splats(n, W, H, seed):
    """The generator of test_gpu_parity.test_forward_bitwise_adversarial."""
    rng = np.random.default_rng(seed)
    s = np.zeros(n, dtype=O.SPLAT_DTYPE)
    s["pos"][:, 0] = rng.uniform(0, W - 1, n)
    s["pos"][:, 1] = rng.uniform(0, H - 1, n)
    s["sx"] = rng.choice([1.0, 1.5, 3.0, 8.0, 40.0, 300.0, 1024.0], n, p=[.15, .15, .3, .3, .06, .03, .01])
    s["sy"] = rng.choice([1.0, 2.0, 6.0, 25.0, 1024.0], n, p=[.2, .3, .4, .09, .01])
    s["rot"] = rng.uniform(-7, 7, n)
    s["color"] = rng.uniform(0, 1, (n, 3))
    s["opacity"] = rng.uniform(0.1, 1.0, n)
    return s


def _trained_state(tgt, W, H, n, steps):
    """Splats and Adam state after `steps` iterations from init()."""
    with S2D.Trainer(W, H, n, deterministic=True) as t:
        t.set_target(tgt)
        t.init()
        if steps:
            t.step(steps, want_mse=False)
        return t.get_splats(), t.get_adam()


def _run(tgt, W, H, splats, adam=None, fused=True, lean=False, **kw):
    """One forward + backward pass of the given state in a fresh context: (image bytes, mse, gradient bytes)."""
    with S2D.Trainer(W, H, len(splats), **kw) as t:
        t.set_target(tgt)
        t.set_splats(splats)
        if adam is not None:
            t.set_adam(*adam)
        t.lean_backward = lean
        if fused:
            t.forward_backward()
        else:
            t.forward()
            t.backward()
        return t.get_image().tobytes(), t.mse(), t.get_grads().tobytes()


def _assert_paths_equal(tgt, W, H, splats, adam=None, **kw):
    """Compact path (fused, and as forward() + backward()) == list-position path, lean_backward off and on.
    Returns the image bytes."""
    img = None
    for lean in (False, True):
        want = _run(tgt, W, H, splats, adam, lean=lean, deterministic=True, count_pairs=True, **kw)
        for fused in (True, False):
            got = _run(tgt, W, H, splats, adam, fused=fused, lean=lean, deterministic=True, **kw)
            assert got[0] == want[0], ("image", lean, fused)
            assert got[1] == want[1], ("mse", lean, fused)
            assert got[2] == want[2], ("grads", lean, fused)
        img = want[0]
    return img


@pytest.mark.parametrize("steps", [0, 5, 30])
def test_compact_path_equals_list_position_path_mini(steps):
    tgt = _target(MINI)
    splats, adam = _trained_state(tgt, 268, 213, 2000, steps)
    _assert_paths_equal(tgt, 268, 213, splats, adam)


def test_compact_path_equals_list_position_path_50k():
    tgt = _target(FULL)
    splats, adam = _trained_state(tgt, 535, 426, 50000, 2)
    _assert_paths_equal(tgt, 535, 426, splats, adam)


@pytest.mark.parametrize("W,H,n,seed", [(96, 80, 300, 3), (130, 50, 500, 6)])
def test_compact_path_equals_list_position_path_adversarial(W, H, n, seed):
    tgt = O.synthetic_target(W, H)
    _assert_paths_equal(tgt, W, H, _random_splats(n, W, H, seed))


def test_compact_path_equals_list_position_path_row_slab():
    tgt = _target(MINI)
    splats, adam = _trained_state(tgt, 268, 213, 2000, 5)
    _assert_paths_equal(tgt, 268, 213, splats, adam, row_begin=64, row_end=144)


def test_compact_path_equals_list_position_path_fp16_images():
    tgt = _fp16(_target(MINI))
    splats, adam = _trained_state(tgt, 268, 213, 2000, 5)
    _assert_paths_equal(tgt, 268, 213, splats, adam, fp16_images=True)


def test_a_second_launch_and_stale_lists_change_nothing():
    """forward_backward() twice in a row on one context, with no Adam step in between: whatever the first launch left
    behind (the handed-over entries, their count per tile, the retirement hints the second launch sizes its batches
    by) does not reach the second one's results.  Then ten Adam steps under lists that are never
    rebuilt (wide margin), at a learning rate that moves the retirement points, so that every launch runs on hints that
    are stale: after each, image and gradients equal a counting context's given the same splats."""
    tgt = _target(MINI)
    W, H, n = 268, 213, 2000
    splats, adam = _trained_state(tgt, W, H, n, 5)
    fresh = _run(tgt, W, H, splats, adam, deterministic=True)
    with S2D.Trainer(W, H, n, deterministic=True, rebin_interval=1000, rebin_margin=48.0, training_rate=0.5) as t:
        t.set_target(tgt)
        t.set_splats(splats)
        t.set_adam(*adam)
        t.forward_backward()
        assert (t.get_image().tobytes(), t.mse(), t.get_grads().tobytes()) == fresh
        # The gradient buffer is zeroed by the Adam step, not by the pass: a second pass adds the same deterministic sums
        # to it once more, and x + x is exact in binary floating point -- twice the first launch's gradients, bit for bit.
        t.forward_backward()
        twice = (2.0 * np.frombuffer(fresh[2], dtype=np.float32)).tobytes()
        assert (t.get_image().tobytes(), t.mse(), t.get_grads().tobytes()) == (fresh[0], fresh[1], twice)
        rebuilds = t.rebuild_count()
        for k in range(10):
            t.adam_step()
            t.forward_backward()
            got = (t.get_image().tobytes(), t.mse(), t.get_grads().tobytes())
            assert t.rebuild_count() == rebuilds, k  # the lists (and everything tied to their positions) are stale but in use
            want = _run(tgt, W, H, t.get_splats(), deterministic=True, count_pairs=True)
            assert got[0] == want[0], ("image", k)
            assert got[1] == want[1], ("mse", k)
            assert got[2] == want[2], ("grads", k)


def _opaque_front_scene():
    """48x48, nine tiles.  Eight large opaque splats (sigma 40: alpha >= 0.69 at the image's corners, 0.31^5 < 1/256)
    retire every tile after its first entries; 200 small ones behind them sit inside the centre tile, four pixels from
    its border: with a binning margin of 8 the neighbouring tiles list them and execute none of them."""
    B = 8
    n = B + 200
    rng = np.random.default_rng(11)
    s = np.zeros(n, dtype=O.SPLAT_DTYPE)
    s["pos"][:B] = 24.0 + rng.uniform(-0.5, 0.5, (B, 2))
    s["sx"][:B] = 40.0
    s["sy"][:B] = 40.0
    s["opacity"][:B] = 1.0
    side = rng.integers(0, 4, n - B)
    along = rng.uniform(20.0, 28.0, n - B)
    near = np.where(side % 2 == 0, 20.0, 28.0)
    s["pos"][B:, 0] = np.where(side < 2, near, along)
    s["pos"][B:, 1] = np.where(side < 2, along, near)
    s["sx"][B:] = 1.0
    s["sy"][B:] = 1.0
    s["opacity"][B:] = rng.uniform(0.3, 1.0, n - B)
    s["rot"] = rng.uniform(-3, 3, n)
    s["color"] = rng.uniform(0, 1, (n, 3))
    return 48, 48, s, dict(rebin_interval=8, rebin_margin=8.0)


def _disjoint_scene():
    """One 16x16 tile holding 70 small disjoint splats of low opacity: every listed entry executes, and the backward
    walk needs more than one batch (two of 64, three of 32 in deterministic mode)."""
    n = 70
    rng = np.random.default_rng(12)
    s = np.zeros(n, dtype=O.SPLAT_DTYPE)
    k = np.arange(n)
    s["pos"][:, 0] = 0.9 + 1.6 * (k % 9)
    s["pos"][:, 1] = 1.0 + 2.0 * (k // 9)
    s["sx"] = 1.0
    s["sy"] = 1.0
    s["opacity"] = rng.uniform(0.05, 0.3, n)
    s["rot"] = rng.uniform(-3, 3, n)
    s["color"] = rng.uniform(0, 1, (n, 3))
    return 16, 16, s, {}


@pytest.mark.parametrize("scene", ["opaque_front", "disjoint"])
def test_the_two_extremes(scene):
    W, H, s, kw = _opaque_front_scene() if scene == "opaque_front" else _disjoint_scene()
    tgt = O.synthetic_target(W, H)
    o = O.OracleTrainer(tgt, len(s))
    o.splats[:] = s
    want = o.forward().copy()
    # the scene is what it claims to be: staged / executed entries of the forward walk, from a counting context
    with S2D.Trainer(W, H, len(s), count_pairs=True, **kw) as t:
        t.set_target(tgt)
        t.set_splats(s)
        t.forward()
        st = t.stats()
        tx, ty, off, _ = t.tile_lists()
    lens = np.diff(off.astype(np.int64))
    if scene == "opaque_front":
        centre = 1 * tx + 1
        assert lens[centre] == len(s)
        assert all(lens[i] >= 50 for i in (centre - 1, centre + 1, centre - tx, centre + tx))  # the small ones, through the margin
        assert st["fwd_staged"] <= 9 * 64                 # every tile retired within its first batch
        assert st["fwd_wave_execs"] <= 9 * 4 * 8          # ... on the eight large splats and nothing else
    else:
        assert list(lens) == [len(s)]
        assert st["fwd_staged"] == len(s)
        assert st["fwd_wave_execs"] >= len(s)             # every entry ran in some wave
    img = _assert_paths_equal(tgt, W, H, s, **kw)
    assert img == want.tobytes()


def test_training_with_list_rebuilds_equals_the_counting_context():
    """40 steps with unscheduled rebuilds (lr = 1 moves splats out of their binned rectangles): parameters and Adam
    moments byte for byte those of a counting context."""
    tgt = _target(MINI)
    res = []
    for count in (False, True):
        with S2D.Trainer(268, 213, 2000, deterministic=True, count_pairs=count, rebin_interval=8, training_rate=1.0) as t:
            t.set_target(tgt)
            t.init()
            t.step(40, want_mse=False)
            assert t.rebuild_count() >= 3
            a, b1, b2, it = t.get_adam()
            res.append((t.get_splats().tobytes(), a.tobytes(), b1, b2, it, t.rebuild_count()))
    assert res[0] == res[1]
