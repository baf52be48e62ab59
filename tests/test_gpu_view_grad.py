"""GPU tests of the backward pass through a view (include/splat2d.h "view gradients"):
s2d_view_backward_device, s2d_view_grads and the differentiable SplatRenderer.render_view.

The yardsticks hold none of the new code:
  * a SECOND CONTEXT of the raster grid's size (out * samples), loaded with the view's records, running s2d_forward and
    s2d_backward_image_grads on the upstream gradient expanded in NumPy (view_grad_ref.expand): in deterministic mode its
    gradients are the bytes s2d_view_grads must return -- same walks, same slots in the same order, and an expansion that is
    exact;
  * the NumPy restatement of the record transform's adjoint (view_grad_ref.adjoint), in bytes;
  * the oracle at the grid size under the unchanged bars of oracle_lib.grad_bars, the expanded upstream pushed through with
    the pseudo-target method of tests/test_image_grads_cpu.py;
  * s2d_forward + s2d_backward for the identity view with the context's own target;
  * finite differences through the operator with the rule of tests/fd_check.py.
Every (view, samples) pair used on scene M keeps the transformed scales inside [1, 1024], the range the parity tests pin the
rasteriser to the oracle on, and each test asserts that first.  The 513-tile-column view and scene A leave that range: there
the library is compared with itself only.
Scenes: 64 x 48, n = 600 (tests/view_ref.py): every tile's list spans several batches, a view has more than one workgroup."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import fd_check as FD
import oracle_lib as O
import test_image_grads_cpu as IG
import view_grad_ref as G
import view_ref as V
from view_grad_cases import (_torch, assert_pinned, check_against_second_context, check_from_target, context, dev, g9, oracle_case,
                             scene, second_context_list_lengths, vkw)

pytestmark = pytest.mark.gpu

S2D = importlib.import_module("2dgaussiansplatting_amd")
W, H, N = V.SRC_W, V.SRC_H, V.N_SPLATS
MINI = os.path.join(O.GOLDEN, "squirrel_cls_mini_268x213.s2di")
E_INVALID, E_NOMEM = 1, 4
F = np.float32
WIDE = ((0.0, 16.0), 128.25, 0.0, (8208, 16))  # 513 tile columns: the generic list builder


# 1 ---------------------------------------------------------------------------------------------------------------------------
# (the second context: view_grad_cases.check_against_second_context)
PAIRS = [(0, 1), (0, 2), (0, 4), (1, 1), (1, 2), (2, 1), (2, 2), (2, 4), (3, 1), (4, 2)]


@pytest.mark.parametrize("k,samples", PAIRS, ids=["v%d_s%d" % (k + 1, s) for k, s in PAIRS])
def test_view_grads_are_the_bytes_of_a_second_context(k, samples):
    check_against_second_context("M", V.VIEWS[k], samples)


def test_view_grads_of_the_adversarial_scene():
    assert_pinned(V.VIEWS[0], 2)
    check_against_second_context("A", V.VIEWS[0], 2, pinned=False)


def test_view_grads_with_dead_rows():
    check_against_second_context("M", V.VIEWS[2], 2, dead=True)


def test_view_grads_without_the_opacity_gradient():
    check_against_second_context("M", V.VIEWS[0], 2, skip=True)


def test_view_grads_with_generic_binning():
    check_against_second_context("M", V.VIEWS[0], 2, generic_binning=True)


def test_view_grads_of_the_wide_view():
    check_against_second_context("M", WIDE, 1, pinned=False)


# 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,samples,dead", [(2, 2, False), (0, 4, False), (2, 1, True)], ids=["v3_s2", "v1_s4", "v3_s1_dead"])
def test_the_adjoint_is_the_restatement_and_accumulates(k, samples, dead):
    view = V.VIEWS[k]
    assert_pinned(view, samples)
    origin, zoom, fv, (ow, oh) = view
    alive = (np.arange(N) % 3 != 0) if dead else None
    up = G.signed_upstream(oh, ow, seed=7)
    with context(scene("M"), deterministic=True) as t:
        if dead:
            t.set_alive(alive)
        u = dev(up)
        gv = g9(t.view_grads(u.data_ptr(), skip_opacity_grad=False, **vkw(view, samples)))
        assert not g9(t.get_grads()).any()                  # the seam stops before the gradient buffer
        t.view_backward_device(u.data_ptr(), skip_opacity_grad=False, **vkw(view, samples))
        once = g9(t.get_grads()).copy()
        t.view_backward_device(u.data_ptr(), skip_opacity_grad=False, **vkw(view, samples))
        twice = g9(t.get_grads()).copy()
    adj = G.adjoint(g9(scene("M")), gv, origin, zoom, fv, samples, alive=alive)
    want = np.zeros_like(adj) + adj                         # the kernel adds into a zeroed buffer
    assert np.abs(want).max() > 0 and np.isfinite(want).all()
    assert once.tobytes() == want.tobytes()
    assert twice.tobytes() == (want + adj).tobytes()
    if dead:
        assert not once[~alive].any()


# 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,samples", [(0, 1), (0, 4), (2, 2)], ids=["v1_s1", "v1_s4", "v3_s2"])
def test_from_target_is_the_upstream_of_view_minus_target(k, samples):
    check_from_target("M", V.VIEWS[k], samples, seed=k + samples)


# 4 ---------------------------------------------------------------------------------------------------------------------------
# (the oracle side: view_grad_cases.oracle_case)
@pytest.mark.parametrize("exact_exp", [False, True], ids=["fp32", "exact_exp"])
@pytest.mark.parametrize("k,samples", [(0, 2), (2, 1)], ids=["v1_s2", "v3_s1"])
def test_view_grads_meet_the_oracle_bars(k, samples, exact_exp):
    assert_pinned(V.VIEWS[k], samples)
    up, w32, dsum, dabs = oracle_case(k, samples, exact_exp)
    with context(scene("M"), exact_exp=exact_exp) as t:
        u = dev(up)
        got = g9(t.view_grads(u.data_ptr(), skip_opacity_grad=False, **vkw(V.VIEWS[k], samples))).copy()
    nz = dabs > 0
    print("\n[view grads] v%d x %d exact_exp=%s: gpu vs exact %.3e, oracle fp32 vs exact %.3e (of sum |terms|)"
          % (k + 1, samples, exact_exp, (np.abs(got - dsum)[nz] / dabs[nz]).max(), (np.abs(w32 - dsum)[nz] / dabs[nz]).max()))
    st = O.grad_bars(got, w32, dsum, dabs)
    print("[view grads] %s" % st)


# 5 ---------------------------------------------------------------------------------------------------------------------------
def test_identity_view_from_the_target_is_forward_backward():
    tgt = O.synthetic_target(W, H)

    def make():
        t = context(scene("M"), deterministic=True)
        t.set_target(tgt)
        return t

    with make() as a, make() as b:
        a.forward()
        a.backward(skip_opacity_grad=False)
        tg = dev(tgt)
        b.view_backward_device(tg.data_ptr(), W, H, from_target=True, skip_opacity_grad=False)
        ga, gb = a.get_grads(), b.get_grads()
        assert np.abs(g9(ga)).max() > 0
        assert ga.tobytes() == gb.tobytes()
        a.adam_step()
        b.adam_step()
        assert a.get_splats().tobytes() == b.get_splats().tobytes()
        assert a.get_adam()[0].tobytes() == b.get_adam()[0].tobytes()
        assert a.get_splats().tobytes() != scene("M").tobytes()


# 6 ---------------------------------------------------------------------------------------------------------------------------
FD_VIEW = G.FD_VIEW   # view 3's transform x 2 on fd_check's 72 x 56 scene


def fd_setup():
    """fd_check's scene, its target and the view's arguments."""
    s, ref = FD.scene()
    assert_pinned(V.VIEWS[2], 2)
    assert V.scales_in_pinned_range(V.view_rows(s.view(O.SPLAT_DTYPE).reshape(-1), (0.0, 0.0), 0.5, 0.75, 2))
    return s, ref, dict(out_width=ref.shape[1] // 2, out_height=ref.shape[0] // 2, **FD_VIEW)


def renderer(ref, n, **kw):
    return importlib.import_module("2dgaussiansplatting_amd.torch_op").SplatRenderer(ref.shape[1], ref.shape[0], n, **kw)


def test_operator_view_and_render_keep_their_own_frames():
    """The generation rule: render_view's backward uploads its parameters, so a pending render() backward draws its frame
    again and still returns the gradient of its own frame; and what render_view records and refuses."""
    torch = _torch()
    s, ref, kw = fd_setup()
    with torch.cuda.stream(torch.cuda.Stream()):
        with renderer(ref, len(s), exact_exp=True, deterministic=True) as r:
            wa = torch.from_numpy(ref).cuda()
            s1 = s.copy()
            s1[:, 0] += 1.5
            s1[:, 5:8] *= 0.5

            def render_loss(p):
                return (r.render(p)[..., :3] * wa[..., :3]).sum()

            def view_loss(p):
                return (r.render_view(p, **kw)[..., :3] * wa[::2, ::2, :3]).sum()

            alone = []
            for fn, par in ((render_loss, s), (view_loss, s1)):
                p = torch.from_numpy(par).cuda().requires_grad_(True)
                fn(p).backward()
                alone.append(p.grad.cpu().numpy().tobytes())
            assert np.frombuffer(alone[1], dtype=F).any() and alone[0] != alone[1]
            pa = torch.from_numpy(s).cuda().requires_grad_(True)
            pb = torch.from_numpy(s1).cuda().requires_grad_(True)
            la = render_loss(pa)
            vb = r.render_view(pb, **kw)
            assert vb.requires_grad and tuple(vb.shape) == (ref.shape[0] // 2, ref.shape[1] // 2, 4)
            (vb[..., :3] * wa[::2, ::2, :3]).sum().backward()   # uploads pb: the frame in the context is no longer pa's
            la.backward()
            assert pb.grad.cpu().numpy().tobytes() == alone[1]
            assert pa.grad.cpu().numpy().tobytes() == alone[0]
            assert not r.render_view(torch.from_numpy(s).cuda(), **kw).requires_grad
            assert r.render_view(torch.from_numpy(s).cuda(), rgba8=True, **kw).dtype == torch.uint8
            with pytest.raises(ValueError):
                r.render_view(pb, rgba8=True, **kw)


def test_operator_view_backward_is_the_derivative():
    """Finite differences through SplatRenderer.render_view under fd_check's bars as they stand (steps, consist 4e-3, rtol
    1e-2, at least 40 and 60 % usable), exact_exp, the loss sum w * view, view 3's transform x 2 so that filter, zoom and
    resolve all act, all nine parameters of the scene's 14 splats.
    The weights are view_grad_ref.fd_weights, formed from the operator's own view: the gradient of the weighted Charbonnier
    loss against the half-size target at the tested point, held fixed.  tests/test_view_grad_cpu.py holds the oracle alone to
    the same check with the same weights (worst 7.9e-3 there) and records the two choices of weights under which the yardstick
    itself misses its bar, on the oracle as on this operator (2.14e-2 and 1.16e-2, both on a rot)."""
    torch = _torch()
    s, ref, kw = fd_setup()
    with torch.cuda.stream(torch.cuda.Stream()):
        with renderer(ref, len(s), exact_exp=True) as r:
            def render(s9):
                return r.render_view(torch.from_numpy(np.ascontiguousarray(s9)).cuda(), **kw).cpu().numpy()

            w3 = G.fd_weights(render(s), G.box_half(ref), IG.charbonnier_grad, IG.charbonnier_weights)
            assert (w3 < 0).any() and (w3 > 0).any() and not w3[:, : kw["out_width"] // 3].any()
            p = torch.from_numpy(s).cuda().requires_grad_(True)
            (r.render_view(p, **kw)[..., :3].double() * torch.from_numpy(w3).cuda().double()).sum().backward()
            g = p.grad.cpu().numpy().astype(np.float64)
            st = IG.check_general(render, lambda im: w3.astype(np.float64) * im[..., :3].astype(np.float64), g, s)
    print("\n[fd] operator view, expf, view 3 x 2: used %d skipped %d worst %.2e at %s"
          % (st["used"], st["skipped"], st["worst_rel"], st["worst_at"]))


# 7 ---------------------------------------------------------------------------------------------------------------------------
def test_view_backward_does_not_interfere_with_training():
    torch = _torch()
    tgt = O.target_rgba32f(O.load_s2di(MINI))[:96, :128].copy()
    view = V.VIEWS[0]
    _, _, _, (ow, oh) = view
    up = dev(G.signed_upstream(oh, ow, seed=3))

    def run(with_views):
        with S2D.Trainer(128, 96, 700, deterministic=True) as t:
            t.set_target(tgt)
            t.init()
            mse1 = t.step(3)
            if with_views:
                before = t.get_image()
                side = torch.zeros((700, 9), dtype=torch.float32, device="cuda")
                torch.cuda.synchronize()
                t.bind_grads(side.data_ptr())
                t.view_backward_device(up.data_ptr(), skip_opacity_grad=False, **vkw(view, 2))
                t.view_backward_device(up.data_ptr(), from_target=True, **vkw(view, 1))
                t.synchronize()
                t.bind_grads(0)                              # its own buffer again
                assert bool(side.any()) and t.get_image().tobytes() == before.tobytes()
            mse2 = t.step(3)
            ad = t.get_adam()
            return (t.get_splats().tobytes(), ad[0].tobytes(), (float(ad[1]), float(ad[2]), ad[3]), mse1.tobytes(), mse2.tobytes(),
                    t.rebuild_count(), t.stats()["rebins"], t.get_image().tobytes())

    plain, viewed = run(False), run(True)
    for a, b in zip(plain, viewed):
        assert a == b


# 8 ---------------------------------------------------------------------------------------------------------------------------
def test_coarse_to_fine_trains():
    tgt = O.target_rgba32f(O.load_s2di(MINI))
    Ht, Wt = tgt.shape[:2]
    hh, hw = Ht // 2, Wt // 2
    t64 = tgt[:2 * hh, :2 * hw].astype(np.float64)
    half = ((t64[0::2, 0::2] + t64[0::2, 1::2] + t64[1::2, 0::2] + t64[1::2, 1::2]) * 0.25).astype(F)

    def mse_of(t):
        t.forward()
        d = (t.get_image()[..., :3].astype(np.float64) - tgt[..., :3]) * 255.0
        return float((d * d).mean())

    def make():
        t = S2D.Trainer(Wt, Ht, 1024, deterministic=True)
        t.set_target(tgt)
        t.init()
        return t

    with make() as a:
        mse0 = mse_of(a)
        hd = dev(half)
        for _ in range(30):
            a.view_backward_device(hd.data_ptr(), hw, hh, zoom=0.5, from_target=True)
            a.adam_step()
        mse30 = mse_of(a)
        end_a = float(a.step(30)[-1])
    with make() as b:
        end_b = float(b.step(60)[-1])
    print("\n[coarse to fine] full-size MSE: start %.2f, after 30 half-size iterations %.2f; end A (30 + 30) %.2f, end B (60 full) %.2f"
          % (mse0, mse30, end_a, end_b))
    assert mse30 < mse0
    assert np.isfinite([mse30, end_a, end_b]).all()


# 9 ---------------------------------------------------------------------------------------------------------------------------
ABI_ROWS = [(k, c, r) for k, (c, r) in enumerate(V.REFUSAL_TABLE)
            if r or dict(V.GOOD, **c)["out_width"] * dict(V.GOOD, **c)["out_height"] <= 1 << 16]


@pytest.fixture(scope="module")
def ctx_m():
    with context(scene("M")) as t:
        yield t


@pytest.fixture(scope="module")
def big_buffer():
    torch = _torch()
    buf = torch.zeros((1 << 16) * 4 + 8, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    return buf


@pytest.mark.parametrize("changes,refused", [(c, r) for _, c, r in ABI_ROWS], ids=[str(k) for k, _, _ in ABI_ROWS])
def test_refusal_table_through_the_abi(ctx_m, big_buffer, changes, refused):
    cfg = V.make_config(S2D._ViewConfig, **dict(changes))
    refused = refused or cfg.format != 0                     # a gradient is RGBA32F
    want = E_INVALID if refused else 0
    out = np.zeros(N, dtype=O.SPLAT_DTYPE)
    ptr = C.c_void_p(big_buffer.data_ptr())
    assert ctx_m.L.s2d_view_grads(ctx_m._h, C.byref(cfg), ptr, 0, O._p(out)) == want
    assert ctx_m.L.s2d_view_backward_device(ctx_m._h, C.byref(cfg), ptr, 0) == want
    assert ctx_m.L.s2d_view_backward_device(ctx_m._h, C.byref(cfg), None, 0) == E_INVALID
    ctx_m.synchronize()


def test_other_refusals(big_buffer):
    good = V.make_config(S2D._ViewConfig)
    out = np.zeros(N, dtype=O.SPLAT_DTYPE)
    base = big_buffer.data_ptr()
    with context(scene("M")) as t:
        L, h = t.L, t._h
        assert L.s2d_view_backward_device(h, None, C.c_void_p(base), 0) == E_INVALID
        assert L.s2d_view_grads(h, C.byref(good), C.c_void_p(base), 0, None) == E_INVALID
        for off, want in ((4, E_INVALID), (8, E_INVALID), (16, 0)):
            assert L.s2d_view_backward_device(h, C.byref(good), C.c_void_p(base + off), 0) == want, off
            assert L.s2d_view_grads(h, C.byref(good), C.c_void_p(base + off), 0, O._p(out)) == want, off
        for flags, want in ((0x1, 0), (0x8, 0), (0x9, 0), (0x2, E_INVALID), (0x4, E_INVALID), (0x10, E_INVALID), (0x80000000, E_INVALID)):
            assert L.s2d_view_backward_device(h, C.byref(good), C.c_void_p(base), flags) == want, flags
        assert b"flags" in L.s2d_last_error(h)
        t.synchronize()
        t.step(2)                                             # and the context trains on
    for kw in ({"count_pairs": True}, {"reference_order": True}):
        with context(scene("M"), **kw) as t:
            assert t.L.s2d_view_backward_device(t._h, C.byref(good), C.c_void_p(base), 0) == E_INVALID
            assert t.L.s2d_view_grads(t._h, C.byref(good), C.c_void_p(base), 0, O._p(out)) == E_INVALID
            t.render_view(**vkw(V.VIEWS[4]))                  # (a view itself is no obstacle there)
    with S2D.Trainer(64, 64, 10, row_begin=16, row_end=48) as slab:
        slab.set_target_synthetic()
        slab.init()
        assert slab.L.s2d_view_backward_device(slab._h, C.byref(good), C.c_void_p(base), 0) == E_INVALID


def test_pair_budget_refuses_and_the_context_trains_on(big_buffer):
    budget = 4000  # view 6 lists every splat with a 40-pixel scale in all of its 60 tiles: > 216 * 60 pairs

    def make():
        t = S2D.Trainer(W, H, N, deterministic=True, chunk_pairs=budget)
        t.set_target_synthetic()
        t.set_splats(scene("M").view(S2D.SPLAT_DTYPE))
        return t

    with make() as t, make() as twin:
        cfg = V.make_config(S2D._ViewConfig, out_width=160, out_height=96, origin_x=20.0, origin_y=10.0, zoom=16.0)
        ptr = C.c_void_p(big_buffer.data_ptr())
        assert t.L.s2d_view_backward_device(t._h, C.byref(cfg), ptr, 0) == E_NOMEM
        assert b"pairs" in t.L.s2d_last_error(t._h)
        assert not g9(t.get_grads()).any()
        a, b = t.step(2), twin.step(2)
        assert a.tobytes() == b.tobytes()
        assert t.get_splats().tobytes() == twin.get_splats().tobytes()
        assert t.get_adam()[0].tobytes() == twin.get_adam()[0].tobytes()
        assert t.get_image().tobytes() == twin.get_image().tobytes()


def test_release_and_calls_of_changing_size():
    ups = {}
    with context(scene("M"), deterministic=True) as t:
        def grads(k, samples):
            _, _, _, (ow, oh) = V.VIEWS[k]
            if (k, samples) not in ups:
                ups[(k, samples)] = dev(G.signed_upstream(oh, ow, seed=k))
            return t.view_grads(ups[(k, samples)].data_ptr(), skip_opacity_grad=False, **vkw(V.VIEWS[k], samples)).tobytes()

        first = grads(0, 1)
        assert np.frombuffer(first, dtype=F).any()
        others = [grads(0, 4), grads(4, 2), grads(5, 1), grads(2, 2)]   # grids of other sizes, lists that grow
        assert grads(0, 1) == first
        t.view_release()
        assert grads(0, 1) == first                                      # allocated again
        assert [grads(0, 4), grads(4, 2), grads(5, 1), grads(2, 2)] == others
        t.view_release()
        t.view_release()                                                 # nothing to free: fine


# 10 --------------------------------------------------------------------------------------------------------------------------
def test_the_scratch_arrives_after_the_lists_and_follows_their_growth():
    """The seam between a view's lists and its raster scratch (RasterSurface::ensure_pairs): a render allocates lists alone, the
    first gradient pass on them brings the scratch to their capacity, lists that grow release it and the next gradient pass
    makes it follow.  One deterministic context on scene M goes through
      (a) render view 1 x 1        (b) view_grads of it: the scratch arrives at an unchanged list capacity
      (c) render view 1 x 4        (d) view_grads of it
    -- each of these is a call on a grid of another size, which creates lists and scratch anew -- and then, on ONE grid (160 x 96
    at 4 samples, the origin of view 6), where lists and scratch live on from call to call:
      (g) view_grads at zoom 0.5: fewer than 65536 pairs, lists of the first capacity and a scratch of it
      (h) render at zoom 16 (view 6): more than 65536 pairs, the lists grow and the scratch goes
      (i) view_grads at zoom 16: the scratch follows the lists
      (j) view_grads at zoom 0.5 again: nothing grows, few pairs in lists and scratch of the large capacity
    and back:
      (e) view_grads of view 1 x 1 again
      (f) step(2)
    Every view call returns the bytes of the same call made first in a fresh context, and (f) leaves the trace, the splats, the
    Adam state and the image of a twin that never drew a view.  No tolerance anywhere.  The pair counts are printed and the two of
    the shared grid asserted to lie on either side of 65536, from the lists a second context builds for the same records and grid
    (view 1 x 4 stays below it: by themselves (a) to (d) grow nothing)."""
    v1, far, near = V.VIEWS[0], (V.VIEWS[5][0], 0.5, 0.0, V.VIEWS[5][3]), V.VIEWS[5]
    pairs = [int(second_context_list_lengths("M", v, s).sum()) for v, s in ((v1, 1), (v1, 4), (far, 4), (near, 4))]
    print("\n[scratch seam] (tile, splat) pairs: view 1 x 1 %d, view 1 x 4 %d; 160 x 96 x 4 at zoom 0.5 %d, at zoom 16 %d" % tuple(pairs))
    assert 0 < pairs[2] <= 1 << 16 < pairs[3]
    ups = {size: dev(G.signed_upstream(size[1], size[0], seed=3)) for size in (v1[3], near[3])}

    def render(t, view, samples):
        return t.render_view(**vkw(view, samples)).tobytes()

    def grads(t, view, samples):
        return t.view_grads(ups[view[3]].data_ptr(), skip_opacity_grad=False, **vkw(view, samples)).tobytes()

    def state(t):
        ad = t.get_adam()
        return (t.get_splats().tobytes(), ad[0].tobytes(), (float(ad[1]), float(ad[2]), ad[3]), t.get_image().tobytes())

    calls = [(render, v1, 1), (grads, v1, 1), (render, v1, 4), (grads, v1, 4),
             (grads, far, 4), (render, near, 4), (grads, near, 4), (grads, far, 4), (grads, v1, 1)]
    want = {}
    for call in calls:                                        # (two of the nine are repeated)
        if call not in want:
            with context(scene("M"), deterministic=True) as fresh:
                want[call] = call[0](fresh, *call[1:])
    assert len(want) == 7 and all(np.frombuffer(w, dtype=F).any() for w in want.values())
    assert want[(grads, far, 4)] != want[(grads, near, 4)]
    with context(scene("M"), deterministic=True) as t, context(scene("M"), deterministic=True) as twin:
        for k, call in enumerate(calls):
            assert call[0](t, *call[1:]) == want[call], (k, call[0].__name__, call[1][1], call[2])
        a, b = t.step(2), twin.step(2)
        assert a.tobytes() == b.tobytes() and np.isfinite(a).all()
        assert state(t) == state(twin)
        assert t.get_splats().tobytes() != scene("M").tobytes()
