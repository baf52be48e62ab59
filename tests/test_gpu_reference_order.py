"""Reference-order validation mode (S2D_CFG_REFERENCE_ORDER, Trainer(reference_order=True)) against the oracle, on bits.

In this mode every backward pass evaluates the nine addends of each (splat, pixel) with the reference's own expressions
and adds each splat's in one fp32 chain in the order of main.cpp:576-598; the squared error is the row-major double
chain of main.cpp:796-805.  So dSplats, the updated splats / splatAdams and every MSE are the oracle's bytes: each
comparison below is np.array_equal on uint32 / uint64 views, without tolerances and without excluded elements.  (The
oracle's gradients on these scenes are all finite -- asserted where they are formed -- so NaN payloads do not arise.)

State of this file: written and collected without a GPU; it had not been run on an MI355X when it was committed
("Not run on a GPU yet").
"""
import functools
import importlib
import json
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from oracle_lib import random_splats
from test_gpu_parity import make_pair, mini_target

pytestmark = pytest.mark.gpu

S2D = importlib.import_module("2dgaussiansplatting_amd")
MINI = os.path.join(O.GOLDEN, "squirrel_cls_mini_268x213.s2di")
KAT = json.load(open(os.path.join(O.GOLDEN, "survey_appendix_c.json")))
ADVERSARIAL = [(16, 16, 40, 5), (33, 17, 64, 4), (96, 80, 300, 3), (130, 50, 500, 6), (1, 1, 5, 7)]


def bits32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same32(got, want):
    return np.array_equal(bits32(got), bits32(want))


def same64(got, want):
    return np.array_equal(np.asarray(got, dtype=np.float64).view(np.uint64), np.asarray(want, dtype=np.float64).view(np.uint64))


def finite(d):
    return bool(np.isfinite(d.view(np.float32)).all())


@functools.lru_cache(maxsize=None)
def adversarial_oracle(W, H, n, seed, exact=False):
    """-> (target, splats, image0, dSplats after one backward pass, after a second one without zeroing, mse)."""
    tgt = O.synthetic_target(W, H)
    o = O.OracleTrainer(tgt, n)
    o.splats[:] = random_splats(n, W, H, seed)
    o.L.s2do_set_exact_exp(1 if exact else 0)
    try:
        img = o.forward().copy()
        d1 = o.backward().copy()
        d2 = o.backward(zero=False).copy()
    finally:
        o.L.s2do_set_exact_exp(0)
    assert finite(d1) and finite(d2)
    return tgt, o.splats.copy(), img, d1, d2, o.mse()


def loaded(W, H, n, tgt, splats, **kw):
    t = S2D.Trainer(W, H, n, reference_order=True, **kw)
    t.set_target(tgt)
    t.set_splats(splats.view(S2D.SPLAT_DTYPE))
    return t


# ---------------------------------------------------------------------------------------------
# 1. adversarial scenes: one tile, sizes that are no multiple of 16, splats whose rectangle spans every tile
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [{}, {"generic_binning": True}], ids=["two_level", "generic_binning"])
@pytest.mark.parametrize("W,H,n,seed", ADVERSARIAL)
def test_adversarial_scenes(W, H, n, seed, kw):
    tgt, splats, img, d1, _, mse = adversarial_oracle(W, H, n, seed)
    with loaded(W, H, n, tgt, splats, **kw) as t:
        t.forward()
        t.backward()
        assert same32(t.get_image(), img)
        assert same32(t.get_grads(), d1)
        assert same64(t.mse(), mse)


def test_adversarial_scene_exact_exp():
    W, H, n, seed = 96, 80, 300, 3
    tgt, splats, img, d1, _, mse = adversarial_oracle(W, H, n, seed, True)
    with loaded(W, H, n, tgt, splats, exact_exp=True) as t:
        t.forward()
        t.backward()
        assert same32(t.get_image(), img)
        assert same32(t.get_grads(), d1)
        assert same64(t.mse(), mse)


def test_flag_combinations_change_nothing():
    """With S2D_CFG_DETERMINISTIC the result is that of reference order alone; S2D_CFG_ADAM_FP32 does not touch gradients."""
    W, H, n, seed = 96, 80, 300, 3
    tgt, splats, _, d1, _, mse = adversarial_oracle(W, H, n, seed)
    with loaded(W, H, n, tgt, splats, deterministic=True, adam_fp32=True) as t:
        t.forward()
        t.backward()
        assert same32(t.get_grads(), d1)
        assert same64(t.mse(), mse)


# ---------------------------------------------------------------------------------------------
# 2. the mini scene: every backward entry point
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mini_oracle(n, steps, opacity):
    o, t = make_pair(mini_target(), n, steps, opacity, reference_order=True)
    t.close()
    img = o.forward().copy()
    d = o.backward().copy()
    assert finite(d)
    return o, img, d, o.mse()


def mini_loaded(o, opacity):
    t = S2D.Trainer(o.W, o.H, o.n, reference_order=True)
    t.set_target(o.ref)
    t.set_splats(o.splats.view(S2D.SPLAT_DTYPE))
    t.set_adam(o.adams.view(S2D.ADAM_DTYPE), o.beta1t[0], o.beta2t[0], o.iterations)
    t.optimize_opacity = opacity
    return t


@pytest.mark.parametrize("n,steps,opacity", [(1024, 0, False), (2000, 5, False), (1024, 30, True)])
def test_mini_scene_every_backward_entry_point(n, steps, opacity):
    import torch
    o, img, want, mse = mini_oracle(n, steps, opacity)
    with mini_loaded(o, opacity) as t:
        t.forward()
        t.backward()
        assert same32(t.get_grads(), want) and same64(t.mse(), mse)
    with mini_loaded(o, opacity) as t:
        t.forward_backward()
        assert same32(t.get_grads(), want) and same64(t.mse(), mse)
        assert same32(t.get_image(), img)
    with mini_loaded(o, opacity) as t:
        t.forward()
        up = torch.from_numpy(np.ascontiguousarray(img - o.ref)).cuda()  # fp32(image0 - ref), main.cpp:616
        torch.cuda.synchronize()
        t.backward_image_grads(up.data_ptr(), skip_opacity_grad=False)
        assert same32(t.get_grads(), want)
    with mini_loaded(o, opacity) as t:
        t.forward()
        t.backward(skip_opacity_grad=True)
        got = t.get_grads().view(np.float32).reshape(-1, 9)
        w9 = want.view(np.float32).reshape(-1, 9)
        assert same32(got[:, :8], w9[:, :8])
        assert not bits32(got[:, 8]).any()
        assert w9[:, 8].any()


# ---------------------------------------------------------------------------------------------
# 3. accumulation, 4. row slabs
# ---------------------------------------------------------------------------------------------
def test_backward_accumulates_like_the_oracle():
    W, H, n, seed = 96, 80, 300, 3
    tgt, splats, _, d1, d2, _ = adversarial_oracle(W, H, n, seed)
    assert not same32(d1, d2)
    with loaded(W, H, n, tgt, splats) as t:
        t.forward()
        t.backward()
        t.backward()
        assert same32(t.get_grads(), d2)


def test_row_slab_contexts():
    W, H, n, seed = 96, 80, 300, 3
    tgt, splats, img, _, _, _ = adversarial_oracle(W, H, n, seed)
    o = O.OracleTrainer(tgt, n)
    o.splats[:] = splats
    o.forward()
    for y0, y1 in ((0, 48), (48, 80)):
        want = o.backward(y0, y1).copy()
        assert finite(want)
        sq = o.L.s2do_sqerr_rows(O._p(o.image0), O._p(o.ref), W, H, y0, y1)
        with loaded(W, H, n, tgt, splats, row_begin=y0, row_end=y1) as t:
            t.forward()
            t.backward()
            assert same32(t.get_image_rows(), img[y0:y1])
            assert same32(t.get_grads(), want)
            assert same64(t.mse(), sq / (H * W * 3))
            assert same64(t.sqerr_trace(0, 1)[0], sq)


# ---------------------------------------------------------------------------------------------
# 5. trajectory: 50 iterations, every MSE and the final state
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_trajectory(opacity):
    """As tests/test_oracle_kat.py run_trace: the opacity checkbox is ticked after the first iteration."""
    o = O.OracleTrainer(mini_target(), 1024)
    tr = []
    for k in range(50):
        if k == 1:
            o.optimize_opacity = opacity
        st, mse = o.step()
        assert st == 0
        tr.append(mse)
    return o, tr


@pytest.mark.parametrize("rebin_interval", [0, 1])
@pytest.mark.parametrize("opacity", [False, True])
def test_trajectory_of_fifty_iterations(opacity, rebin_interval):
    o, want = oracle_trajectory(opacity)
    with S2D.Trainer(o.W, o.H, 1024, reference_order=True, rebin_interval=rebin_interval) as t:
        t.set_target(o.ref)
        t.init()
        got = []
        for k in range(50):
            if k == 1:
                t.optimize_opacity = opacity
            got.append(t.step(1)[0])
        for k in range(50):
            assert same64(got[k], want[k]), (k, got[k], want[k])
        assert same32(t.get_splats(), o.splats)
        adams, b1, b2, it = t.get_adam()
        assert same32(adams, o.adams)
        assert same32(np.float32(b1), o.beta1t[0]) and same32(np.float32(b2), o.beta2t[0])
        assert it == o.iterations == 50


# ---------------------------------------------------------------------------------------------
# 6. the survey's known-answer traces, no oracle involved
# ---------------------------------------------------------------------------------------------
def kat_lines(name):
    k = KAT[name]
    out = {int(i): v for i, v in k["mse_at"].items()}
    out.update({i: v for i, v in enumerate(k.get("mse_0_to_11", []))})
    return out


@pytest.mark.parametrize("name,opacity", [("mini_n1024_as_shipped", False),
                                          ("mini_n1024_optimize_opacity_from_iteration_1", True)])
def test_golden_trace(name, opacity):
    with S2D.Trainer(268, 213, 1024, reference_order=True) as t:
        t.set_target(mini_target())
        t.init()
        if opacity:
            tr = list(t.step(1))
            t.optimize_opacity = True
            tr += list(t.step(299))
        else:
            tr = list(t.step(300))
    want = kat_lines(name)
    assert {0, 1, 100, 299} <= set(want) and (opacity or set(range(12)) | {199} <= set(want))
    assert {k: "%.4f" % tr[k] for k in want} == want


def test_cpp_host_prints_the_golden_trace():
    exe = S2D._build.build_host_program()
    r = subprocess.run([exe, "--image", MINI, "--splats", "1024", "--iters", "300", "--reference-order"], capture_output=True,
                       text=True, check=True)
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 300
    want = kat_lines("mini_n1024_as_shipped")
    assert {k: lines[k] for k in want} == {k: "%d itr, mse %s" % (k, v) for k, v in want.items()}  # main.cpp:807


# ---------------------------------------------------------------------------------------------
# 7. what the mode refuses, 8. what it leaves alone
# ---------------------------------------------------------------------------------------------
def test_refusals(monkeypatch):
    for kw in ({"count_pairs": True}, {"fp16_images": True}):
        with pytest.raises(S2D.S2DError) as e:
            S2D.Trainer(16, 16, 40, reference_order=True, **kw)
        assert e.value.code == 1  # S2D_E_INVALID
    with pytest.raises(S2D.S2DError) as e:
        S2D.MultiTrainer(96, 80, 300, [0], share_gpu=True, reference_order=True)
    assert e.value.code == 1
    W, H, n, seed = 96, 80, 300, 3
    tgt, splats, _, _, _, _ = adversarial_oracle(W, H, n, seed)
    with loaded(W, H, n, tgt, splats, chunk_pairs=100) as t:  # the scene has more pairs: it would need index ranges
        with pytest.raises(S2D.S2DError) as e:
            t.forward()
        assert e.value.code == 4 and "S2D_CFG_REFERENCE_ORDER" in str(e.value)  # S2D_E_NOMEM
    with S2D.Trainer(W, H, n, reference_order=True) as t:  # slab ownership
        import torch
        masks = torch.ones(n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        with pytest.raises(S2D.S2DError) as e:
            t.halo_commit(masks.data_ptr(), 0)
        assert e.value.code == 1
    monkeypatch.setenv("S2D_REFERENCE_ORDER_MAX_BYTES", "1048576")
    with pytest.raises(S2D.S2DError) as e:
        S2D.Trainer(16, 16, 40, reference_order=True)  # (the binding destroys the context it was handed)
    assert e.value.code == 4
    assert "1048576" in str(e.value) and str(65536 * 9 * 256 * 4) in str(e.value)  # the bound, and the minimum capacity's bytes
    with S2D.Trainer(16, 16, 40) as t:  # the bound concerns no other context
        t.set_target_synthetic()
        t.init()
        t.forward()


def test_default_mode_untouched():
    W, H, n, seed = 96, 80, 300, 3
    tgt, splats, img, d1, _, _ = adversarial_oracle(W, H, n, seed)
    with S2D.Trainer(W, H, n) as t:
        t.set_target(tgt)
        t.set_splats(splats.view(S2D.SPLAT_DTYPE))
        t.forward()
        t.backward()
        assert same32(t.get_image(), img)
        assert not same32(t.get_grads(), d1)  # atomic order and the fast path's regrouped terms: equal bits would be a surprise
    with loaded(W, H, n, tgt, splats) as t:
        t.forward()
        assert same32(t.get_image(), img)
