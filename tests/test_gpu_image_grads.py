"""GPU tests of the backward pass from a caller's image gradient (s2d_backward_image_grads), of the device-pointer calls
around it (s2d_set_splats_device, s2d_get_image_rows_device) and of the PyTorch operator on top (torch_op.SplatRenderer).

Two yardsticks, both independent of the new code:
  * s2d_backward itself: the upstream gradient fp32(image0 - imageRef), formed OUTSIDE the kernel, is bit for bit what
    the kernel forms at main.cpp:616 (a lone fp32 subtraction has one result), so in deterministic mode the new pass
    must reproduce s2d_backward's gradients -- and the Adam step behind them -- byte for byte, in every variant;
  * the oracle, for an upstream gradient that is no squared-error gradient at all (masked, signed: the weighted
    Charbonnier loss of tests/test_image_grads_cpu.py, where the method is pinned on the CPU), under the unchanged
    gradient bars of oracle_lib.grad_bars, and by finite differences through the operator itself.
Device buffers are torch tensors.  A plain Trainer works on a stream of its own, so these tests synchronise both sides
between torch's work and the library's; the operator shares torch's stream and needs none.
"""
import functools
import importlib
import os

import numpy as np
import pytest

import fd_check as FD
import oracle_lib as O
import test_image_grads_cpu as IG

pytestmark = pytest.mark.gpu

S2D = importlib.import_module("2dgaussiansplatting_amd")
MINI = os.path.join(O.GOLDEN, "squirrel_cls_mini_268x213.s2di")
N = 2000
REL = 1e-4  # as tests/test_gpu_parity.py


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
    return t.get_grads().view(np.float32).reshape(-1, 9)


@functools.lru_cache(maxsize=None)
def mini_state():
    """The mini scene with the oracle advanced 3 steps (make_pair of tests/test_gpu_parity.py): target, splats, Adam state."""
    tgt = O.target_rgba32f(O.load_s2di(MINI))
    o = O.OracleTrainer(tgt, N)
    for _ in range(3):
        o.step()
    return tgt, o.splats.copy(), o.adams.copy(), float(o.beta1t[0]), float(o.beta2t[0]), o.iterations


def mini_trainer(**kw):
    tgt, splats, adams, b1, b2, it = mini_state()
    t = S2D.Trainer(tgt.shape[1], tgt.shape[0], N, **kw)
    t.set_target(tgt)
    t.set_splats(splats.view(S2D.SPLAT_DTYPE))
    t.set_adam(adams.view(S2D.ADAM_DTYPE), b1, b2, it)
    return t


def image_on_device(t):
    """image0 of the context's rows as s2d_get_image_rows_device returns it: (rows, W, 4) float32 tensor."""
    torch = _torch()
    img = torch.empty((t.row_end - t.row_begin, t.W, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    t.get_image_rows_device(img.data_ptr())
    t.synchronize()
    return img


def assert_same_bits_as_backward(make, ref_rows, skip):
    """make() -> a loaded Trainer (deterministic).  One runs forward(); backward(); the other forward(), forms
    fp32(image0 - ref) in torch and runs backward_image_grads: same gradient bytes, and the same bytes after adam_step()."""
    torch = _torch()
    with make() as a, make() as b:
        a.forward()
        a.backward(skip_opacity_grad=skip)
        b.forward()
        img = image_on_device(b)
        assert img.cpu().numpy().tobytes() == b.get_image_rows().tobytes()
        up = img - dev(ref_rows)
        torch.cuda.synchronize()
        b.backward_image_grads(up.data_ptr(), skip_opacity_grad=skip)
        ga, gb = a.get_grads(), b.get_grads()
        assert np.abs(ga.view(np.float32)).max() > 0
        assert ga.tobytes() == gb.tobytes()
        if skip:
            assert not gb["opacity"].any()
        a.adam_step()
        b.adam_step()
        assert a.get_splats().tobytes() == b.get_splats().tobytes()
        assert a.get_adam()[0].tobytes() == b.get_adam()[0].tobytes()


# ---------------------------------------------------------------------------------------------
# 1. the same bits as s2d_backward
# ---------------------------------------------------------------------------------------------
CASES = {"plain": {}, "fp16_images": {"fp16_images": True}, "slab": {"row_begin": 64, "row_end": 160},
         "index_ranges": {"chunk_pairs": 3000}, "generic_binning": {"generic_binning": True}}


@pytest.mark.parametrize("skip", [False, True], ids=["opacity", "skip_opacity"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_upstream_of_the_squared_error_gives_the_bits_of_backward(case, skip):
    kw = CASES[case]
    tgt = mini_state()[0]
    ref = tgt[kw.get("row_begin", 0):kw.get("row_end", tgt.shape[0])]
    if kw.get("fp16_images"):
        ref = ref.astype(np.float16).astype(np.float32)  # what the context keeps of the target (round to nearest even)
    assert_same_bits_as_backward(lambda: mini_trainer(deterministic=True, **kw), ref, skip)


# ---------------------------------------------------------------------------------------------
# 2., 3. an arbitrary upstream gradient against the oracle
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def charbonnier_case():
    """Oracle side, computed once: image0, the upstream gradient as the oracle forms it, and its gradient statistics."""
    tgt, splats = mini_state()[:2]
    o = O.OracleTrainer(tgt, N)
    o.splats[:] = splats
    img = o.forward().copy()
    g = IG.charbonnier_grad(img, tgt, IG.charbonnier_weights(*tgt.shape[:2]))
    pseudo = IG.pseudo_target(img, g)
    o.ref = np.ascontiguousarray(pseudo)
    w32, dsum, dabs = o.backward_stats()
    up = IG.upstream_of(img, pseudo)
    assert (up[..., :3] < 0).any() and (up[..., :3] > 0).any() and not up[:, : tgt.shape[1] // 3].any()
    return img, up, w32.view(np.float32).reshape(-1, 9).copy(), dsum, dabs


@pytest.mark.parametrize("kw", [{}, {"chunk_pairs": 2000}], ids=["plain", "index_ranges"])
def test_arbitrary_upstream_meets_the_oracle_bars(kw):
    img, up, w32, dsum, dabs = charbonnier_case()
    with mini_trainer(**kw) as t:
        t.forward()
        assert t.get_image().tobytes() == img.tobytes()
        u = dev(up)
        t.backward_image_grads(u.data_ptr(), skip_opacity_grad=False)
        got = g9(t).copy()
    st = O.grad_bars(got, w32, dsum, dabs, REL)
    assert int((dabs == 0).sum()) > 0  # (the masked third: scalars that must be exactly zero exist)
    print("\n[image grads] %s: %s" % (kw, st))


def test_slab_contexts_add_up_under_an_upstream_gradient():
    D = importlib.import_module("2dgaussiansplatting_amd.distributed")
    img, up, w32, dsum, dabs = charbonnier_case()
    with mini_trainer() as full:
        full.forward()
        u = dev(up)
        full.backward_image_grads(u.data_ptr(), skip_opacity_grad=False)
        g_full = g9(full).astype(np.float64)
    g = np.zeros((N, 9), dtype=np.float64)
    for rank in range(2):
        r0, r1 = D.slab_rows(img.shape[0], rank, 2)
        with mini_trainer(row_begin=r0, row_end=r1) as t:
            t.forward()
            u = dev(up[r0:r1])
            t.backward_image_grads(u.data_ptr(), skip_opacity_grad=False)
            g += g9(t)
    nz = dabs > 0
    assert (np.abs(g - dsum)[nz] / dabs[nz]).max() <= 1e-6
    assert (np.abs(g - g_full)[nz] / dabs[nz]).max() <= 1e-6
    assert np.all(g[~nz] == 0)


# ---------------------------------------------------------------------------------------------
# 4. edge cases
# ---------------------------------------------------------------------------------------------
def test_zero_upstream_gives_zero_gradients():
    torch = _torch()
    with mini_trainer(deterministic=True) as t:
        t.forward()
        u = torch.zeros((t.H, t.W, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        t.backward_image_grads(u.data_ptr(), skip_opacity_grad=False)
        assert not g9(t).any()


def test_the_fourth_channel_of_the_upstream_is_ignored():
    up = charbonnier_case()[1]
    out = []
    for w in (0.0, np.nan):
        with mini_trainer(deterministic=True) as t:
            t.forward()
            v = up.copy()
            v[..., 3] = w
            v[::3, ::5, 3] = 7.5
            u = dev(v)
            t.backward_image_grads(u.data_ptr(), skip_opacity_grad=False)
            out.append(t.get_grads().tobytes())
    assert out[0] == out[1] and np.frombuffer(out[0], dtype=np.float32).any()
    assert np.isfinite(np.frombuffer(out[1], dtype=np.float32)).all()


@pytest.mark.parametrize("W,H", [(40, 1), (17, 33)])
def test_partial_tiles_give_the_bits_of_backward(W, H):
    rng = np.random.default_rng(W * 100 + H)
    n = 12
    s = np.zeros((n, 9), dtype=np.float32)
    s[:, 0] = rng.uniform(0, W, n)
    s[:, 1] = rng.uniform(0, H, n)
    s[:, 2:4] = rng.uniform(1.5, 6.0, (n, 2))
    s[:, 4] = rng.uniform(0, np.pi, n)
    s[:, 5:8] = rng.uniform(0.1, 0.9, (n, 3))
    s[:, 8] = rng.uniform(0.25, 0.9, n)
    tgt = O.synthetic_target(W, H)

    def make():
        t = S2D.Trainer(W, H, n, deterministic=True)
        t.set_target(tgt)
        t.set_splats(s.view(S2D.SPLAT_DTYPE).reshape(-1))
        return t

    assert_same_bits_as_backward(make, tgt, False)


# ---------------------------------------------------------------------------------------------
# 5., 6. the operator
# ---------------------------------------------------------------------------------------------
def _op():
    return importlib.import_module("2dgaussiansplatting_amd.torch_op")


def charbonnier_torch(img, ref, w):
    torch = _torch()
    d = img[..., :3].double() - ref[..., :3]
    return (w[..., None] * torch.sqrt(d * d + IG.CHARB_EPS ** 2)).sum()


@pytest.mark.parametrize("deterministic", [False, True])
def test_operator_backward_is_the_derivative_of_a_charbonnier_loss(deterministic):
    torch = _torch()
    s, ref = FD.scene()
    H, W = ref.shape[:2]
    w = IG.charbonnier_weights(H, W)
    with torch.cuda.stream(torch.cuda.Stream()):
        with _op().SplatRenderer(W, H, len(s), exact_exp=True, deterministic=deterministic) as r:
            p = torch.from_numpy(s).cuda().requires_grad_(True)
            loss = charbonnier_torch(r.render(p), torch.from_numpy(ref).cuda().double(), torch.from_numpy(w).cuda())
            loss.backward()
            g = p.grad.cpu().numpy().astype(np.float64)
            assert g.shape == (len(s), 9)

            def render(s9):
                with torch.no_grad():
                    return r.render(torch.from_numpy(np.ascontiguousarray(s9)).cuda()).cpu().numpy()

            st = IG.check_general(render, lambda im: IG.charbonnier_terms(im, ref, w), g, s)
    print("\n[fd] operator, expf, weighted Charbonnier, deterministic=%s: used %d skipped %d worst %.2e at %s"
          % (deterministic, st["used"], st["skipped"], st["worst_rel"], st["worst_at"]))


def test_operator_squared_error_gives_the_bits_of_backward():
    torch = _torch()
    tgt, splats = mini_state()[:2]
    with mini_trainer(deterministic=True) as t:
        t.forward()
        t.backward(skip_opacity_grad=False)
        want_img, want = t.get_image(), t.get_grads().tobytes()
    with torch.cuda.stream(torch.cuda.Stream()):
        with _op().SplatRenderer(tgt.shape[1], tgt.shape[0], N, deterministic=True) as r:
            p = torch.from_numpy(splats.view(np.float32).reshape(-1, 9).copy()).cuda().requires_grad_(True)
            ref = torch.from_numpy(tgt).cuda()
            img = r.render(p)
            loss = 0.5 * ((img[..., :3] - ref[..., :3]) ** 2).sum()
            loss.backward()
            assert img.detach().cpu().numpy().tobytes() == want_img.tobytes()
            assert p.grad.cpu().numpy().tobytes() == want


def test_operator_backward_calls_in_reverse_order_get_their_own_frames():
    torch = _torch()
    tgt, splats = mini_state()[:2]
    s0 = splats.view(np.float32).reshape(-1, 9).copy()
    s1 = s0.copy()
    s1[:, 0] += 3.0
    s1[:, 5:8] *= 0.5
    with torch.cuda.stream(torch.cuda.Stream()):
        ref = torch.from_numpy(tgt).cuda()

        def loss_of(img):
            return (img[..., :3] - ref[..., :3]).abs().sum()

        with _op().SplatRenderer(tgt.shape[1], tgt.shape[0], N, deterministic=True) as r:
            single = []
            for s in (s0, s1):
                p = torch.from_numpy(s).cuda().requires_grad_(True)
                loss_of(r.render(p)).backward()
                single.append(p.grad.cpu().numpy().tobytes())
            assert single[0] != single[1]
            pa = torch.from_numpy(s0).cuda().requires_grad_(True)
            pb = torch.from_numpy(s1).cuda().requires_grad_(True)
            la = loss_of(r.render(pa))
            lb = loss_of(r.render(pb))
            lb.backward()   # the frame in the context is pb's
            la.backward()   # ... and no longer pa's: the operator has to draw pa again
            assert pb.grad.cpu().numpy().tobytes() == single[1]
            assert pa.grad.cpu().numpy().tobytes() == single[0]


def test_operator_trains_an_l1_loss_with_torch_adam():
    torch = _torch()
    tgt, splats = mini_state()[:2]
    with torch.cuda.stream(torch.cuda.Stream()):
        ref = torch.from_numpy(tgt).cuda()
        with _op().SplatRenderer(tgt.shape[1], tgt.shape[0], N) as r:
            p = torch.nn.Parameter(torch.from_numpy(splats.view(np.float32).reshape(-1, 9).copy()).cuda())
            opt = torch.optim.Adam([p], lr=0.01)
            losses = []
            for _ in range(30):
                opt.zero_grad()
                loss = (r.render(p)[..., :3] - ref[..., :3]).abs().mean()
                loss.backward()
                opt.step()
                losses.append(loss.detach())
            losses = [float(v) for v in torch.stack(losses).cpu()]
            assert bool(torch.isfinite(p).all())
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
    print("\n[operator] L1, torch Adam, 30 steps: %.5f -> %.5f" % (losses[0], losses[-1]))


def test_operator_refuses_another_stream_and_other_tensors():
    torch = _torch()
    s, ref = FD.scene()
    with torch.cuda.stream(torch.cuda.Stream()):
        r = _op().SplatRenderer(ref.shape[1], ref.shape[0], len(s))
        p = torch.from_numpy(s).cuda()
        assert tuple(r.render(p).shape) == (ref.shape[0], ref.shape[1], 4)
        with pytest.raises(ValueError):
            r.render(p.double())
        with pytest.raises(ValueError):
            r.render(p[:, :8])
        torch.cuda.current_stream().synchronize()
    with torch.cuda.stream(torch.cuda.Stream()):
        with pytest.raises(RuntimeError):
            r.render(p)
    r.close()


# ---------------------------------------------------------------------------------------------
# 7. the device-pointer calls
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [{}, {"fp16_images": True}, {"row_begin": 64, "row_end": 160}], ids=["fp32", "fp16", "slab"])
def test_get_image_rows_device_returns_the_bytes_of_get_image_rows(kw):
    with mini_trainer(**kw) as t:
        t.forward()
        img = image_on_device(t)
        want = t.get_image_rows()
        assert want.any() and img.cpu().numpy().tobytes() == want.tobytes()


@pytest.mark.parametrize("shift,rebuilds", [(0.25, False), (40.0, True)], ids=["small_move", "out_of_the_rectangle"])
def test_set_splats_device_equals_set_splats_on_a_fresh_context(shift, rebuilds):
    splats = mini_state()[1]
    moved = splats.view(np.float32).reshape(-1, 9).copy()
    moved[:, 0:2] += np.float32(shift)
    with mini_trainer(deterministic=True) as fresh:
        fresh.set_splats(moved.view(S2D.SPLAT_DTYPE).reshape(-1))
        fresh.forward()
        fresh.backward(skip_opacity_grad=False)
        want_img, want_g = fresh.get_image().tobytes(), fresh.get_grads().tobytes()
    with mini_trainer(deterministic=True) as t:
        t.forward()  # lists of the unmoved splats
        before = t.rebuild_count()
        m = dev(moved)
        t.set_splats_device(m.data_ptr())
        t.forward()
        t.backward(skip_opacity_grad=False)
        assert t.get_splats().tobytes() == moved.tobytes()
        assert t.get_image().tobytes() == want_img
        assert t.get_grads().tobytes() == want_g
        assert (t.rebuild_count() > before) == rebuilds


# ---------------------------------------------------------------------------------------------
# 8. call order
# ---------------------------------------------------------------------------------------------
def test_call_order_and_argument_errors():
    torch = _torch()
    tgt = mini_state()[0]
    u = torch.zeros((tgt.shape[0], tgt.shape[1], 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with mini_trainer() as t:
        with pytest.raises(S2D.S2DError) as e:
            t.backward_image_grads(u.data_ptr())          # no forward yet
        assert e.value.code == 5
        t.forward_backward(skip_image=True)
        with pytest.raises(S2D.S2DError) as e:
            t.backward_image_grads(u.data_ptr())          # image0 is not this frame's
        assert e.value.code == 5
        t.forward()
        with pytest.raises(S2D.S2DError) as e:
            t.backward_image_grads(u.data_ptr() + 4)      # not 16-byte aligned
        assert e.value.code == 1
        with pytest.raises(S2D.S2DError) as e:
            t.backward_image_grads(0)
        assert e.value.code == 1
        t.backward()
        mse = t.mse()
        t.backward_image_grads(u.data_ptr())
        assert t.mse() == mse and mse > 0
    with mini_trainer(count_pairs=True) as t:
        t.forward()
        with pytest.raises(S2D.S2DError) as e:
            t.backward_image_grads(u.data_ptr())
        assert e.value.code == 1
