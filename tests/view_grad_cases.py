"""What the GPU tests of the view gradients share (tests/test_gpu_view_grad.py, tests/test_gpu_view_variants.py): the scenes by
name, a context loaded with one, and the three yardsticks that hold none of the view gradient code --
  * check_against_second_context: a SECOND CONTEXT of the raster grid's size (out * samples), loaded with the view's records,
    running s2d_forward and s2d_backward_image_grads on the upstream gradient expanded in NumPy (view_grad_ref.expand); in
    deterministic mode its gradients are the bytes s2d_view_grads must return;
  * check_from_target: S2D_VIEW_BWD_FROM_TARGET against the same context's s2d_view_grads fed view - target, formed in fp32 on
    the device;
  * oracle_case / oracle_side: the oracle at the grid size, the upstream of the weighted Charbonnier loss of the VIEW pushed
    through with the pseudo-target method of tests/test_image_grads_cpu.py, for the bars of oracle_lib.grad_bars.
The oracle sides are computed once per case and never written afterwards.  Nothing here needs a GPU to be imported."""
import functools
import importlib

import numpy as np

import oracle_lib as O
import test_image_grads_cpu as IG
import view_grad_ref as G
import view_ref as V

F = np.float32


def _s2d():
    return importlib.import_module("2dgaussiansplatting_amd")


def _torch():
    import torch
    return torch


def dev(a):
    """numpy -> device tensor, complete before the library's stream may read it."""
    torch = _torch()
    a = np.ascontiguousarray(a)
    x = torch.from_numpy(a if a.flags.writeable else a.copy()).cuda()   # (the shared oracle sides are read-only)
    torch.cuda.synchronize()
    return x


def _scene_m_out_of_range_colours():
    """Scene M with the out-of-range colours of tests/test_gpu_view.py::test_rgba8_is_the_quantiser_of_the_float_view, 1.5 and
    -0.2, by channel instead of by region: red 1.5 and blue -0.2 in every splat, green as it is.  View 1 is decided by the
    first two dozen splats, scales of 100 pixels that every pixel blends, so colouring regions of the source leaves the view
    on one side of [0, 1] only (computed with the oracle: that test's regions, pos.x < 24 and > 40, give no pixel below 0, and
    neither does a split at any column from 6 to 24 give both); by channel, both clamps work in every covered pixel and green keeps values to round."""
    s = V.scene_m().copy()
    s["color"][:, 0] = 1.5
    s["color"][:, 2] = -0.2
    return s


SCENES = {"M": V.scene_m, "A": V.scene_a, "S": V.scene_sparse, "Mc": _scene_m_out_of_range_colours}


@functools.lru_cache(maxsize=None)
def scene(name):
    return SCENES[name]()


def context(splats, width=V.SRC_W, height=V.SRC_H, **kw):
    S2D = _s2d()
    t = S2D.Trainer(width, height, len(splats), **kw)
    t.set_target_synthetic()
    t.set_splats(np.ascontiguousarray(splats).view(S2D.SPLAT_DTYPE))
    return t


def vkw(view, samples=1):
    origin, zoom, fv, (ow, oh) = view
    return dict(out_width=ow, out_height=oh, origin=origin, zoom=zoom, filter_var=fv, samples=samples)


def assert_pinned(view, samples, name="M"):
    origin, zoom, fv, _ = view
    assert V.scales_in_pinned_range(V.view_rows(scene(name), origin, zoom, fv, samples))


def g9(a):
    return G.rows9(a)


# ---- the second context ------------------------------------------------------------------------------------------------------
def second_context_grads(records, gw, gh, upstream, skip, alive=None, **kw):
    with context(records, gw, gh, deterministic=True, **kw) as t2:
        if alive is not None:
            t2.set_alive(alive)
        t2.forward()
        u = dev(upstream)
        t2.backward_image_grads(u.data_ptr(), skip_opacity_grad=skip)
        return t2.get_grads()


def second_context_list_lengths(name, view, samples):
    """The lengths of the tile lists of the view's raster grid, read through the second context: the same records, the same
    grid and the same builder.  rebin_interval=1: a training context inflates its rectangles by a re-use margin (2 pixels
    and more, include/splat2d.h) unless it rebuilds its lists every iteration; a view projects with margin 0 (DESIGN.md section
    17), and so does this context.  (With the default margin the lists are longer than the view's: scene M through view 1
    352 to 413 entries, and the sparse scene at one sample per axis has no tile with exactly one entry.)"""
    origin, zoom, fv, (ow, oh) = view
    with context(V.view_rows(scene(name), origin, zoom, fv, samples), ow * samples, oh * samples, deterministic=True,
                 rebin_interval=1) as t2:
        t2.forward()
        tx, ty, off, _ = t2.tile_lists()
    lengths = np.diff(off.astype(np.int64))
    assert len(lengths) == tx * ty == ((ow * samples + 15) // 16) * ((oh * samples + 15) // 16)
    return lengths


def check_against_second_context(name, view, samples, skip=False, dead=False, pinned=True, **kw):
    """-> the gradients s2d_view_grads returned (structured), after the asserts."""
    if pinned:
        assert_pinned(view, samples, name)
    origin, zoom, fv, (ow, oh) = view
    alive = (np.arange(len(scene(name))) % 3 != 0) if dead else None
    up = G.signed_upstream(oh, ow, seed=samples)
    assert (up < 0).any() and not up[:, : ow // 3].any()
    with context(scene(name), deterministic=True, **kw) as t:
        if dead:
            t.set_alive(alive)
        records = t.view_splats(ow, oh, origin, zoom, fv, samples)
        u = dev(up)
        got = t.view_grads(u.data_ptr(), skip_opacity_grad=skip, **vkw(view, samples))
        again = t.view_grads(u.data_ptr(), skip_opacity_grad=skip, **vkw(view, samples))
    want = second_context_grads(records, ow * samples, oh * samples, G.expand(up, samples), skip, alive, **kw)
    assert np.abs(g9(want)).max() > 0
    assert got.tobytes() == want.tobytes()
    assert again.tobytes() == got.tobytes()  # the buffer is zeroed per call, the slots are re-stamped
    if skip:
        assert not got["opacity"].any()
    if dead:
        assert not g9(got)[~alive].any()
    return got


# ---- from the target ---------------------------------------------------------------------------------------------------------
def check_from_target(name, view, samples, seed, skip=False, pinned=True, **kw):
    """-> the gradients s2d_view_grads returned from the target (structured), after the asserts."""
    torch = _torch()
    if pinned:
        assert_pinned(view, samples, name)
    _, _, _, (ow, oh) = view
    tgt = np.random.default_rng(seed).uniform(0, 1, (oh, ow, 4)).astype(F)
    with context(scene(name), deterministic=True, **kw) as t:
        tg = dev(tgt)
        img = torch.empty((oh, ow, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        t.render_view_device(img.data_ptr(), **vkw(view, samples))
        t.synchronize()
        up = img - tg                                       # fp32, one subtraction per channel
        torch.cuda.synchronize()
        want = t.view_grads(up.data_ptr(), skip_opacity_grad=skip, **vkw(view, samples))
        got = t.view_grads(tg.data_ptr(), from_target=True, skip_opacity_grad=skip, **vkw(view, samples))
    assert np.abs(g9(want)).max() > 0
    assert got.tobytes() == want.tobytes()
    return got


# ---- the oracle --------------------------------------------------------------------------------------------------------------
def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def _oracle_at_grid(name, view, samples):
    origin, zoom, fv, (ow, oh) = view
    rows = V.view_rows(scene(name), origin, zoom, fv, samples)
    gw, gh = ow * samples, oh * samples
    o = O.OracleTrainer(O.synthetic_target(gw, gh), len(rows))
    o.splats[:] = rows
    return o


@functools.lru_cache(maxsize=None)
def oracle_side(name, view, samples, exact_exp):
    """Oracle side, once per case: the records at the grid size, the upstream gradient of the VIEW and the statistics of the
    oracle's backward pass from its expansion (pseudo-target method).
    The upstream is the one the method was pinned with (tests/test_image_grads_cpu.py, tests/test_gpu_image_grads.py): the
    gradient of the weighted Charbonnier loss of the view against a target of its size -- masked on a third of the columns,
    signed, and spatially coherent as the gradient of an image loss is.  The last property is what gives bar (b) of grad_bars
    its meaning: the bar compares the worst scalar of the GPU's sums with the worst scalar of the reference's sequential fp32
    sums, and the latter grows with the number of like-signed terms of a splat.  Under white noise (the upstream of the byte
    tests) every sum cancels, the reference's worst scalar stays near one rounding (1.29e-7 of sum |terms| on v3 x 1)
    and a splat with a single term, whose few-ulp regrouping error grad_bars' docstring allows, decides the GPU's
    (1.74e-7): the bar then ranks roundings, not summation.
    -> {image: the oracle's frame at the grid size, resolved: its resolve (the view), fwd: the forward counters (visited,
    active), up, w32, dsum, dabs}."""
    _, _, _, (ow, oh) = view
    o = _oracle_at_grid(name, view, samples)
    O.lib().s2do_set_exact_exp(1 if exact_exp else 0)
    try:
        fc = O.Counters()
        img = o.forward(counters=fc).copy()
        resolved = V.resolve(img, samples)
        up = IG.charbonnier_grad(resolved, O.synthetic_target(ow, oh), IG.charbonnier_weights(oh, ow))
        assert (up[..., :3] < 0).any() and (up[..., :3] > 0).any() and not up[:, : ow // 3].any()
        pseudo = IG.pseudo_target(img, G.expand(up, samples))
        if samples == 1:
            up = IG.upstream_of(img, pseudo)                # the bits the oracle forms at main.cpp:616
        o.ref = np.ascontiguousarray(pseudo)
        w32, dsum, dabs = o.backward_stats()
    finally:
        O.lib().s2do_set_exact_exp(0)
    return _frozen({"image": img, "resolved": resolved, "fwd": (fc.visited, fc.active), "up": up,
                    "w32": w32.view(np.float32).reshape(-1, 9).copy(), "dsum": dsum, "dabs": dabs})


def oracle_case(k, samples, exact_exp):
    """oracle_side of scene M through V.VIEWS[k] -> (up, w32, dsum, dabs)."""
    r = oracle_side("M", V.VIEWS[k], samples, exact_exp)
    return r["up"], r["w32"], r["dsum"], r["dabs"]


@functools.lru_cache(maxsize=None)
def oracle_side_from_target(name, view, samples, exact_exp):
    """The same for S2D_VIEW_BWD_FROM_TARGET, whose upstream the kernel forms itself: fp32 (view - target) per channel.  With g
    the Charbonnier gradient of oracle_side, the target is T = fp32(resolved - g), so that the upstream u = fp32(resolved - T)
    is g up to one rounding: signed, coherent, and exactly 0 on the masked third (T = resolved there).  The oracle is handed
    the expansion of u as its pseudo-target; at samples = 1 that is the oracle's own backward pass with target T.
    -> {target: T, up: u, w32, dsum, dabs}; the view the kernel subtracts T from must be `resolved` in bytes, which the caller
    asserts."""
    _, _, _, (ow, oh) = view
    side = oracle_side(name, view, samples, exact_exp)
    img, resolved = side["image"], side["resolved"]
    g = IG.charbonnier_grad(resolved, O.synthetic_target(ow, oh), IG.charbonnier_weights(oh, ow))
    target = IG.pseudo_target(resolved, g)
    up = IG.upstream_of(resolved, target)
    assert (up[..., :3] < 0).any() and (up[..., :3] > 0).any() and not up[:, : ow // 3].any()
    o = _oracle_at_grid(name, view, samples)
    O.lib().s2do_set_exact_exp(1 if exact_exp else 0)
    try:
        assert o.forward().tobytes() == img.tobytes()
        o.ref = np.ascontiguousarray(target if samples == 1 else IG.pseudo_target(img, G.expand(up, samples)))
        w32, dsum, dabs = o.backward_stats()
    finally:
        O.lib().s2do_set_exact_exp(0)
    return _frozen({"target": target, "up": up, "w32": w32.view(np.float32).reshape(-1, 9).copy(), "dsum": dsum, "dabs": dabs})
