"""GPU tests of the seams between the context's owners (2dgaussiansplatting_amd/csrc/s2d_context.h) and of the one step
driver behind s2d_step and s2d_step_loss: the non-finite tail of both entry points, the two ways a call reads its
squared-error trace, and one context that leaves index-range rendering and comes back to it.

Everything is compared on bytes between routes of the library itself, in deterministic mode, so no tolerance is involved.
"""
import ctypes as C
import importlib

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

S2D = importlib.import_module("2dgaussiansplatting_amd")
E_NONFINITE = 3


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def test_nonfinite_tail_is_the_same_through_step_and_step_loss():
    """From one state with an infinite first moment, s2d_step and s2d_step_loss (squared error alone, then all three
    terms) stop at the same iteration, report it alike and end their traces alike: one value, then NaN."""
    W, H, n = 64, 48, 300
    with S2D.Trainer(W, H, n, deterministic=True) as t:
        t.set_target_synthetic()
        t.init()
        t.step(3)
        splats = t.get_splats()
        ad, b1, b2, it = t.get_adam()
    assert it == 3
    ad["mv"][7, 4, 0] = np.inf      # first moment of splat 7's rot: its next update is non-finite

    def run(weights):
        with S2D.Trainer(W, H, n, deterministic=True) as t:
            t.set_target_synthetic()
            t.set_splats(splats)
            t.set_adam(ad, b1, b2, it)
            mse, loss = np.zeros(6), np.zeros(6)
            if weights is None:
                loss = None
                rc = t.L.s2d_step(t._h, 6, 0, _vp(mse))
            else:
                cfg = t._loss_config(*weights)
                rc = t.L.s2d_step_loss(t._h, 6, 0, C.byref(cfg), _vp(loss), _vp(mse))
            _, b1f, b2f, itf = t.get_adam()
            return rc, mse, loss, (itf, b1f.tobytes(), b2f.tobytes()), t.stats()["first_nonfinite_iteration"]

    rc_s, mse_s, _, counters_s, first_s = run(None)
    rc_l, mse_l, loss_l, counters_l, first_l = run((1.0, 0.0, 0.0))
    print("mse", mse_s, mse_l, "loss", loss_l, "counters", counters_s[0], counters_l[0])
    assert rc_s == E_NONFINITE and rc_l == E_NONFINITE
    assert np.isfinite(mse_s[0]) and np.isnan(mse_s[1:]).all()
    assert mse_s.tobytes() == mse_l.tobytes()
    assert np.array_equal(np.isnan(loss_l), np.isnan(mse_l))
    assert counters_s == counters_l and counters_s[0] == 4
    assert first_s == 3 and first_l == 3
    rc_m, mse_m, loss_m, counters_m, first_m = run((1.0, 0.2, 0.2))
    print("mixed loss", loss_m, "mse", mse_m)
    assert rc_m == E_NONFINITE and first_m == 3 and counters_m == counters_s
    assert np.array_equal(np.isnan(mse_m), np.isnan(mse_s)) and np.array_equal(np.isnan(loss_m), np.isnan(mse_s))
    assert np.isfinite(loss_m[0])


def test_trace_reads_on_both_sides_of_the_pinned_buffer_agree():
    """4100 iterations in one call (more than the 4096 doubles of the pinned buffer: the trace is read by itself), as
    4096 + 4 (each call reads trace and status word in one round trip), and as 4100 x (forward_backward, adam_step) with
    the trace read afterwards: the same MSE values, splats and moments."""
    W, H, n, total = 32, 32, 8, 4100

    def run(route):
        with S2D.Trainer(W, H, n, deterministic=True) as t:
            t.set_target_synthetic()
            t.init()
            if route == "one_call":
                mse = t.step(total)
            elif route == "two_calls":
                mse = np.concatenate([t.step(4096), t.step(total - 4096)])
            else:
                for _ in range(total):
                    t.forward_backward(skip_opacity_grad=True)   # (what s2d_step asks for while "Optimize opacity" is off)
                    t.adam_step()
                mse = t.sqerr_trace(0, total) / (3.0 * W * H)
                t.synchronize()
            ad, b1, b2, it = t.get_adam()
            return mse, t.get_splats().tobytes(), ad.tobytes(), (it, b1.tobytes(), b2.tobytes())

    one, two, passes = run("one_call"), run("two_calls"), run("passes")
    print("mse first", one[0][0], "last", one[0][-1])
    assert np.isfinite(one[0]).all() and one[3][0] == total
    for other, name in ((two, "4096 + 4"), (passes, "separate passes")):
        assert other[0].tobytes() == one[0].tobytes(), name
        assert other[1:] == one[1:], name


def _small_scene(W, H, n, shift=0.0):
    rng = np.random.default_rng(41)
    s = np.zeros(n, dtype=O.SPLAT_DTYPE)
    s["pos"][:, 0] = rng.uniform(4, W - 5, n) + shift
    s["pos"][:, 1] = rng.uniform(4, H - 5, n) + shift
    s["sx"] = rng.uniform(0.4, 0.6, n)
    s["sy"] = rng.uniform(0.4, 0.6, n)
    s["rot"] = rng.uniform(0, np.pi, n)
    s["color"] = rng.uniform(0, 1, (n, 3))
    s["opacity"] = rng.uniform(0.3, 0.9, n)
    return s


def _covering_scene(W, H, n):
    rng = np.random.default_rng(42)
    s = np.zeros(n, dtype=O.SPLAT_DTYPE)
    s["pos"][:, 0] = rng.uniform(0, W - 1, n)
    s["pos"][:, 1] = rng.uniform(0, H - 1, n)
    s["sx"] = rng.uniform(250, 400, n)
    s["sy"] = rng.uniform(250, 400, n)
    s["rot"] = rng.uniform(0, np.pi, n)
    s["color"] = rng.uniform(0, 1, (n, 3))
    s["opacity"] = 0.02
    return s


def test_one_context_from_plain_lists_to_index_ranges_and_back():
    """Small splats (one set of lists, re-used), then splats that cover every tile (three index ranges per pass), then
    small splats again, on ONE context with a pair budget: every phase gives what a fresh context gives from the same
    state, with the budget and without."""
    W, H, n, budget = 96, 80, 300, 3000
    kw = dict(deterministic=True, rebin_interval=8)
    A, B, A2 = _small_scene(W, H, n), _covering_scene(W, H, n), _small_scene(W, H, n, shift=1.0)

    def pairs_of(scene):
        with S2D.Trainer(W, H, n, **kw) as t:
            t.set_target_synthetic()
            t.set_splats(scene)
            t.forward()
            return t.stats()["pairs_binned"]

    pa, pb = pairs_of(A), pairs_of(B)
    print("pairs: small", pa, "covering", pb)
    assert pa <= budget < pb and pb == 30 * n        # what this test rests on

    def phase(t, k, scene):
        """-> what the phase left, the list builds of its parts, its final optimiser state, the pair capacity after each part."""
        r0 = t.stats()["rebins"]
        t.set_splats(scene)
        out, builds, capacity = [], [], []

        def part_done():
            st = t.stats()
            builds.append(st["rebins"] - r0 - sum(builds))
            capacity.append(st["pairs_capacity"])

        if k == 2:
            t.forward()
            out.append(t.get_image().tobytes())
            part_done()
            t.backward()
            out.append(t.get_grads().tobytes())
            part_done()
            t.adam_step()
            out.append(t.step(3).tobytes())
        else:
            out.append(t.step(10).tobytes())
        part_done()
        ad, b1, b2, it = t.get_adam()
        out += [t.get_splats().tobytes(), ad.tobytes(), (it, b1.tobytes(), b2.tobytes())]
        return out, builds, (ad, b1, b2, it), capacity

    def fresh(k, scene, start, chunk_pairs):
        with S2D.Trainer(W, H, n, chunk_pairs=chunk_pairs, **kw) as t:
            t.set_target_synthetic()
            if start is not None:
                t.set_splats(scene)                  # (phase() sets them again)
                t.set_adam(*start)
            return phase(t, k, scene)[:2]

    with S2D.Trainer(W, H, n, chunk_pairs=budget, **kw) as t:
        t.set_target_synthetic()
        start, capacities = None, []
        for k, scene in ((1, A), (2, B), (3, A2)):
            got, builds, end, capacity = phase(t, k, scene)
            capacities += capacity
            with_budget, builds_a = fresh(k, scene, start, budget)
            without, builds_b = fresh(k, scene, start, None)
            print("phase", k, "builds", builds, "fresh with budget", builds_a, "without", builds_b, "capacity", capacity)
            assert got == with_budget, "phase %d against a fresh context with the budget" % k
            assert got == without, "phase %d against a fresh context without a budget" % k
            if k == 2:
                # A pass that walks every range builds at least two more sets of lists than one set would take: the
                # forward pass and the backward pass behind it.  The Adam step then clamps every opacity up to 0.1
                # (main.cpp's constraint), 100 such splats saturate every pixel (0.9^100 < 1/256), and a pass stops behind
                # its first range: one build per iteration in step(3), where the context without a budget re-uses its
                # lists and builds none -- lists_valid stays false behind a pass over ranges.
                assert builds[0] >= 2 and builds[1] >= 2 and builds[2] >= 3
                assert builds_b[0] == 1 and builds_b[1] == 0 and builds_b[2] < builds[2]
            if k == 3:
                assert builds == builds_a
            start = end
        assert capacities == sorted(capacities)      # the pair buffers never shrink
