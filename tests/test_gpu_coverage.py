"""GPU tests of the coverage channel (S2D_CFG_COVERAGE).

The yardstick is the WHITE TWIN (tests/coverage_ref.py): a plain context -- no flag -- with the same splats coloured (1, 0, 0).
Coverage is the reference's colour sum for a channel whose colour is 1, so the twin's red channel is the coverage channel
operation for operation, in the forward walk ((T * 1) * alpha), in the backward walk (T * 1 - S / (1 - alpha + 1e-15)) and in a
view -- and the twin runs the kernels that tests/test_gpu_parity.py and tests/test_gpu_raster_variants.py hold to the oracle.
So every bit of the new channel is compared with `==`; only where one more addend changes a rounding (a mixed upstream) is
there a bar, the project's bar (a) of oracle_lib.grad_bars: 1e-6 of the summed magnitudes of the terms, which the oracle reports.

Scenes (coverage_ref.scene): the squirrel mini with 2000 splats, 17 x 17 with 40 splats, 48 x 48 with a stack of 64 large splats
of opacity 0.9.  Over them coverage has pixels that are exactly 0, pixels in (0.05, 0.95) and pixels above 0.99
(coverage_ref.assert_scenes_are_not_trivial, asserted by every test that draws a scene).
"""
import functools
import importlib

import numpy as np
import pytest

import coverage_ref as CR
import test_image_grads_cpu as IG

pytestmark = pytest.mark.gpu

S2D = importlib.import_module("2dgaussiansplatting_amd")
GEOM = [0, 1, 2, 3, 4, 8]   # pos.xy, sx, sy, rot, opacity: what the coverage reaches
COLOUR = [5, 6, 7]


def _torch():
    import torch
    return torch


def dev(a):
    """numpy -> device tensor, complete before the library's stream may read it."""
    torch = _torch()
    x = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return x


def g9(t):
    return t.get_grads().view(np.float32).reshape(-1, 9).copy()


def make(name, twin=False, **kw):
    """A Trainer with the scene's target and splats (twin: coloured (1, 0, 0))."""
    tgt, s9 = CR.scene(name)
    s9 = CR.white_twin(s9) if twin else s9
    t = S2D.Trainer(tgt.shape[1], tgt.shape[0], len(s9), **kw)
    t.set_target(tgt)
    t.set_splats(np.ascontiguousarray(s9).view(S2D.SPLAT_DTYPE).reshape(-1))
    return t


def same_floats(a, b):
    """a == b elementwise as floats: a zero's sign may differ, nothing else."""
    return a.shape == b.shape and bool(np.all(a == b))


def backward_from(t, up, skip):
    t.forward()
    u = dev(up)
    t.backward_image_grads(u.data_ptr(), skip_opacity_grad=skip)
    return g9(t)


@functools.lru_cache(maxsize=None)
def upstreams(name):
    """Oracle side of a scene, once: (rgb0, a0, dabs): the upstream (r, g, b, 0) of the weighted Charbonnier loss as the oracle
    forms it (tests/test_image_grads_cpu.py's pseudo-target construction), the upstream (0, 0, 0, u) with a signed, spatially
    varying u, and the summed magnitudes of the oracle's terms of the two passes -- the plain scene under the first, the white
    twin under (u, 0, 0, .) -- added up."""
    CR.assert_scenes_are_not_trivial()
    tgt, s9 = CR.scene(name)
    H, W = tgt.shape[:2]
    img, twin_img = CR.oracle_frames(name)
    o = CR.oracle_of(tgt, s9)
    o.forward()
    pseudo = IG.pseudo_target(img, IG.charbonnier_grad(img, tgt, IG.charbonnier_weights(H, W)))
    o.ref = np.ascontiguousarray(pseudo)
    dabs_rgb = o.backward_stats()[2].copy()
    rgb0 = IG.upstream_of(img, pseudo)
    u = CR.signed_upstream(H, W)
    ot = CR.oracle_of(tgt, CR.white_twin(s9))
    ot.forward()
    gu = np.zeros(img.shape, dtype=np.float32)
    gu[..., 0] = u
    pseudo_t = IG.pseudo_target(twin_img, gu)
    ot.ref = np.ascontiguousarray(pseudo_t)
    dabs_a = ot.backward_stats()[2].copy()
    ured = IG.upstream_of(twin_img, pseudo_t)[..., 0]   # the bits the oracle formed
    a0 = np.zeros(img.shape, dtype=np.float32)
    a0[..., 3] = ured
    assert rgb0[..., :3].any() and (ured < 0).any() and (ured > 0).any() and not rgb0[..., 3].any()
    return rgb0, a0, dabs_rgb + dabs_a


# ---------------------------------------------------------------------------------------------
# 1. forward
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("name", CR.SCENES)
def test_forward_rgb_is_the_plain_image_and_w_is_the_white_twins_red(name, fp16):
    CR.assert_scenes_are_not_trivial()
    with make(name, coverage=True, fp16_images=fp16) as c, make(name, fp16_images=fp16) as p, make(name, twin=True, fp16_images=fp16) as w:
        for t in (c, p, w):
            t.forward()
        ic, ip, iw = c.get_image(), p.get_image(), w.get_image()
    assert ic[..., :3].tobytes() == ip[..., :3].tobytes()
    assert ic[..., 3].tobytes() == iw[..., 0].tobytes()
    assert (ip[..., 3] == 1).all() and ic[..., 3].any()
    if not fp16:  # (and the twin is the oracle's, bit for bit)
        assert ic[..., 3].tobytes() == CR.oracle_frames(name)[1][..., 0].tobytes()


# ---------------------------------------------------------------------------------------------
# 2. backward, deterministic contexts
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("skip", [False, True], ids=["opacity", "skip_opacity"])
@pytest.mark.parametrize("name", CR.SCENES)
def test_backward_columns_equal_the_plain_context_and_the_white_twin(name, skip, fp16):
    rgb0, a0, _ = upstreams(name)
    kw = dict(deterministic=True, fp16_images=fp16)
    # (r, g, b, 0): all nine columns of a plain context fed the same rgb
    with make(name, coverage=True, **kw) as c, make(name, **kw) as p:
        gc, gp = backward_from(c, rgb0, skip), backward_from(p, rgb0, skip)
    assert gp.any() and same_floats(gc, gp)
    # (0, 0, 0, u): the geometric columns of the white twin fed (u, 0, 0, .); no colour gradient at all
    ured = np.zeros_like(a0)
    ured[..., 0] = a0[..., 3]
    ured[..., 3] = 7.5  # (ignored by a plain context)
    with make(name, coverage=True, **kw) as c, make(name, twin=True, **kw) as w:
        gc, gw = backward_from(c, a0, skip), backward_from(w, ured, skip)
    assert gw[:, GEOM[:5]].any() and same_floats(gc[:, GEOM], gw[:, GEOM])
    assert np.all(gc[:, COLOUR] == 0) and gw[:, 5].any()
    assert (not gc[:, 8].any()) if skip else gc[:, 8].any()


# ---------------------------------------------------------------------------------------------
# 3. mixed upstream
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("det", [False, True], ids=["atomics", "deterministic"])
@pytest.mark.parametrize("name", CR.SCENES)
def test_mixed_upstream_is_the_sum_of_its_parts_to_summation_accuracy(name, det):
    """g(r, g, b, u) against g(r, g, b, 0) + g(0, 0, 0, u), relative to the two oracle passes' summed |terms|.  The only
    difference is the rounding of one more addend in the channel sum, at most 2 ulp per term or 1.2e-7 of the terms'
    magnitudes: well inside bar (a) of oracle_lib.grad_bars, 1e-6, which fp32 summation order already needs."""
    rgb0, a0, dabs = upstreams(name)
    mixed = rgb0.copy()
    mixed[..., 3] = a0[..., 3]
    assert mixed[..., :3].tobytes() == rgb0[..., :3].tobytes() and mixed[..., 3].tobytes() == a0[..., 3].tobytes()
    with make(name, coverage=True, deterministic=det) as c:
        g_mixed = backward_from(c, mixed, False).astype(np.float64)
    parts = np.zeros_like(g_mixed)
    for up in (rgb0, a0):
        with make(name, coverage=True, deterministic=det) as c:
            parts += backward_from(c, up, False)
    nz = dabs > 0
    assert nz.any() and np.abs(parts[nz]).max() > 0
    assert np.all(g_mixed[~nz] == 0) and np.all(parts[~nz] == 0)
    worst = float((np.abs(g_mixed - parts)[nz] / dabs[nz]).max())
    print("\n[coverage] %s %s: max |g(rgbu) - g(rgb0) - g(000u)| / dabs = %.3e" % (name, "det" if det else "atomics", worst))
    assert worst <= 1e-6, worst


def oracle_dabs(name, up):
    """Summed |terms| of the two oracle passes an upstream (r, g, b, u) splits into: the plain scene under (r, g, b), the white
    twin under (u, 0, 0), both through the pseudo-target construction (a scale for summation-order bars, nothing else)."""
    tgt, s9 = CR.scene(name)
    img, twin_img = CR.oracle_frames(name)
    total = 0.0
    for frame, splats, g in ((img, s9, up[..., :3]), (twin_img, CR.white_twin(s9), up[..., 3:])):
        o = CR.oracle_of(tgt, splats)
        o.forward()
        g4 = np.zeros(frame.shape, dtype=np.float32)
        g4[..., :g.shape[-1]] = g
        o.ref = np.ascontiguousarray(IG.pseudo_target(frame, g4))
        total = total + o.backward_stats()[2]
    return total


@pytest.mark.parametrize("from_target", [False, True], ids=["upstream", "target"])
@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("skip", [False, True], ids=["opacity", "skip_opacity"])
def test_every_backward_variant_with_atomics_meets_its_deterministic_twin(skip, fp16, from_target):
    """The sixteen backward kernels, NEED_OP x HALF x DET x UPSTREAM: the eight deterministic ones are held to bits above and in
    4.; each of the eight with float atomics adds the same terms in another order, so it must meet the deterministic kernel of
    the same variant within bar (a) of oracle_lib.grad_bars, 1e-6 of the summed |terms| (the oracle's, fp32 images; with fp16
    images the frames differ from the oracle's by a rounding, which the scale does not notice)."""
    name = "tiny"
    tgt = CR.scene(name)[0]
    rgb0, a0, _ = upstreams(name)
    up = rgb0.copy()
    up[..., 3] = a0[..., 3]
    got = []
    for det in (True, False):
        with make(name, coverage=True, deterministic=det, fp16_images=fp16) as c:
            c.forward()
            if from_target:
                img = c.get_image()
                c.backward(skip_opacity_grad=skip)
            else:
                u = dev(up)
                c.backward_image_grads(u.data_ptr(), skip_opacity_grad=skip)
            got.append(g9(c).astype(np.float64))
    dabs = oracle_dabs(name, (img - tgt).astype(np.float32) if from_target else up)
    nz = dabs > 0
    assert np.abs(got[0][nz]).max() > 0 and np.all(got[0][~nz] == 0) and np.all(got[1][~nz] == 0)
    worst = float((np.abs(got[0] - got[1])[nz] / dabs[nz]).max())
    print("\n[coverage] tiny skip=%s fp16=%s from_target=%s: max |atomics - deterministic| / dabs = %.3e" % (skip, fp16, from_target, worst))
    assert worst <= 1e-6, worst
    assert (not got[1][:, 8].any()) if skip else got[1][:, 8].any()


# ---------------------------------------------------------------------------------------------
# 4. s2d_backward from an RGBA target
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("skip", [False, True], ids=["opacity", "skip_opacity"])
@pytest.mark.parametrize("name", CR.SCENES)
def test_backward_from_the_target_is_the_upstream_image0_minus_target_on_four_channels(name, skip):
    CR.assert_scenes_are_not_trivial()
    tgt = CR.scene(name)[0]
    assert len(np.unique(tgt[..., 3])) > 10  # an alpha worth fitting: the upload must have kept it
    with make(name, coverage=True, deterministic=True) as a, make(name, coverage=True, deterministic=True) as b, make(name) as p:
        a.forward()
        a.backward(skip_opacity_grad=skip)
        b.forward()
        up = (b.get_image() - tgt).astype(np.float32)
        assert up[..., 3].any()
        u = dev(up)
        b.backward_image_grads(u.data_ptr(), skip_opacity_grad=skip)
        ga, gb = g9(a), g9(b)
        p.forward()
        p.backward()
        assert a.mse() == p.mse() and p.mse() > 0   # the squared error stays the three-channel quantity
    assert ga.any() and same_floats(ga, gb)
    # ... and the alpha of the target matters: another alpha, other gradients
    with make(name, coverage=True, deterministic=True) as a2:
        t2 = tgt.copy()
        t2[..., 3] = 1.0
        a2.set_target(t2)
        a2.forward()
        a2.backward(skip_opacity_grad=skip)
        assert not same_floats(g9(a2), ga)


# ---------------------------------------------------------------------------------------------
# 5. s2d_step and s2d_forward_backward
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opacity", [False, True], ids=["fixed_opacity", "optimize_opacity"])
def test_step_is_forward_backward_adam_and_forward_backward_is_forward_then_backward(opacity):
    name = "mini"
    CR.assert_scenes_are_not_trivial()
    with make(name, coverage=True, deterministic=True) as a, make(name, coverage=True, deterministic=True) as b:
        a.optimize_opacity = b.optimize_opacity = opacity
        frame = None
        for _ in range(3):
            a.step(1)
            b.forward()
            frame = b.get_image()
            b.backward(skip_opacity_grad=not opacity)
            b.adam_step()
        assert a.get_splats().tobytes() == b.get_splats().tobytes()
        assert a.get_adam()[0].tobytes() == b.get_adam()[0].tobytes()
        assert a.get_adam()[3] == b.get_adam()[3] == 3
        assert a.get_image().tobytes() == frame.tobytes() and frame[..., 3].any()   # image0 is current after a step
        a.forward_backward(skip_opacity_grad=False, skip_image=True)             # (accepted, no effect)
        b.forward()
        b.backward(skip_opacity_grad=False)
        assert g9(a).any() and a.get_grads().tobytes() == b.get_grads().tobytes()
        assert a.get_image().tobytes() == b.get_image().tobytes()
        assert a.mse() == b.mse()


# ---------------------------------------------------------------------------------------------
# 6. training
# ---------------------------------------------------------------------------------------------
def test_training_fits_an_opaque_disc_on_transparent_black():
    W = H = 64
    y, x = np.mgrid[0:H, 0:W]
    inside = ((x + 0.5 - 32) ** 2 + (y + 0.5 - 30) ** 2) <= 18.0 ** 2
    tgt = np.zeros((H, W, 4), dtype=np.float32)
    tgt[inside] = (0.9, 0.5, 0.2, 1.0)
    with S2D.Trainer(W, H, 256, coverage=True) as t:
        t.set_target(tgt)
        t.init()
        t.optimize_opacity = True
        t.forward()
        img0 = t.get_image()
        t.step(60)
        t.forward()
        img1 = t.get_image()
    sa = [float(((im[..., 3].astype(np.float64) - tgt[..., 3]) ** 2).sum()) for im in (img0, img1)]
    mse = [float(((im[..., :3].astype(np.float64) - tgt[..., :3]) ** 2).mean()) for im in (img0, img1)]
    print("\n[coverage] disc, 60 iterations: sum (A - A_ref)^2 %.3f -> %.3f, rgb mse %.6f -> %.6f" % (sa[0], sa[1], mse[0], mse[1]))
    assert sa[1] < sa[0] and mse[1] < mse[0]


# ---------------------------------------------------------------------------------------------
# 7. views
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mini", "tiny"])
def test_identity_view_is_image0_with_its_coverage(name):
    CR.assert_scenes_are_not_trivial()
    with make(name, coverage=True) as c:
        c.forward()
        img = c.get_image()
        view = c.render_view(c.W, c.H)
    assert img[..., 3].any() and view.tobytes() == img.tobytes()


@pytest.mark.parametrize("rgba8", [False, True], ids=["rgba32f", "rgba8"])
@pytest.mark.parametrize("samples", [1, 2, 4])
@pytest.mark.parametrize("name", ["mini", "tiny"])
def test_zoomed_view_rgb_is_the_plain_view_and_w_is_the_white_twins_red(name, samples, rgba8):
    CR.assert_scenes_are_not_trivial()
    tgt = CR.scene(name)[0]
    H, W = tgt.shape[:2]
    view = dict(out_width=37, out_height=29, origin=(W * 0.21, H * 0.17), zoom=1.7, filter_var=0.3, samples=samples, rgba8=rgba8)
    with make(name, coverage=True) as c, make(name) as p, make(name, twin=True) as w:
        vc, vp, vw = (t.render_view(**view) for t in (c, p, w))
    CR.check_view_against_white_twin(vc, vp, vw, rgba8)


# ---------------------------------------------------------------------------------------------
# 8. torch
# ---------------------------------------------------------------------------------------------
def test_operator_gradient_of_the_summed_coverage_is_the_white_twins_summed_red():
    torch = _torch()
    op = importlib.import_module("2dgaussiansplatting_amd.torch_op")
    tgt, s9 = CR.scene("mini")
    H, W = tgt.shape[:2]
    with torch.cuda.stream(torch.cuda.Stream()):
        with op.SplatRenderer(W, H, len(s9), coverage=True, deterministic=True) as rc, op.SplatRenderer(W, H, len(s9), deterministic=True) as rp:
            pc = torch.from_numpy(np.array(s9)).cuda().requires_grad_(True)
            pw = torch.from_numpy(CR.white_twin(s9)).cuda().requires_grad_(True)
            ic = rc.render(pc)
            iw = rp.render(pw)
            assert ic[..., 3].detach().cpu().numpy().tobytes() == iw[..., 0].detach().cpu().numpy().tobytes()
            ic[..., 3].sum().backward()
            iw[..., 0].sum().backward()
            gc, gw = pc.grad.cpu().numpy(), pw.grad.cpu().numpy()
    assert gw[:, GEOM].any() and same_floats(gc[:, GEOM], gw[:, GEOM]) and np.all(gc[:, COLOUR] == 0)


# ---------------------------------------------------------------------------------------------
# 9. refusals
# ---------------------------------------------------------------------------------------------
def test_refused_calls_answer_invalid_and_touch_nothing():
    torch = _torch()
    name = "mini"
    tgt = CR.scene(name)[0]
    H, W = tgt.shape[:2]
    buf = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    masks = torch.zeros(CR.N_MINI, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    view = dict(out_width=32, out_height=32)
    with make(name, coverage=True) as t:
        t.forward()
        t.backward()
        before = (t.get_grads().tobytes(), t.get_image().tobytes(), t.get_adam()[3])
        assert np.frombuffer(before[0], dtype=np.float32).any()
        refused = [
            lambda: t.backward(density_stats=True),
            lambda: t.backward_image_grads(buf.data_ptr(), density_stats=True),
            lambda: t.step(1, density_stats=True),
            lambda: t.loss_backward(1.0, 0.0, 0.0),
            lambda: t.step_loss(1, 1.0, 0.0, 0.0),
            lambda: t.loss_image_grads_device(buf.data_ptr(), 1.0, 0.0, 0.0),
            lambda: t.view_backward_device(buf.data_ptr(), **view),
            lambda: t.view_grads(buf.data_ptr(), **view),
            lambda: t.halo_masks([0, 112, H], 2.0, masks.data_ptr()),
            lambda: t.halo_commit(masks.data_ptr(), 0),
            lambda: t.halo_commit(0, 0),
        ]
        for k, call in enumerate(refused):
            with pytest.raises(S2D.S2DError) as e:
                call()
            assert e.value.code == S2D.S2D_E_INVALID, k
            assert "S2D_CFG_COVERAGE" in str(e.value), (k, str(e.value))
        assert (t.get_grads().tobytes(), t.get_image().tobytes(), t.get_adam()[3]) == before
    for kw in (dict(count_pairs=True), dict(exact_exp=True), dict(reference_order=True), dict(row_begin=16, row_end=64)):
        with pytest.raises(S2D.S2DError) as e:
            S2D.Trainer(W, H, 16, coverage=True, **kw)
        assert e.value.code == S2D.S2D_E_INVALID


def test_a_scene_beyond_one_set_of_lists_answers_nomem_at_forward():
    with make("mini", coverage=True, chunk_pairs=2000) as t:
        with pytest.raises(S2D.S2DError) as e:
            t.forward()
        assert e.value.code == S2D.S2D_E_NOMEM and "S2D_CFG_COVERAGE" in str(e.value)
        with pytest.raises(S2D.S2DError) as e:
            t.step(1)
        assert e.value.code == S2D.S2D_E_NOMEM
        assert t.get_adam()[3] == 0
    with make("mini", chunk_pairs=2000) as t:  # (the plain context renders the same scene by index ranges)
        t.forward()
        assert t.get_image()[..., :3].any()
