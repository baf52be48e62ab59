"""The events that make a context's derived state stale (2dgaussiansplatting_amd/csrc/s2d_sequence.h), one case each.

A context re-uses its tile lists (rebin_interval=1000) and has run forward, backward, one Adam step and a forward.  Then
the event happens, and three things are observed:

  * what the event's row of the table claims, through status codes and rebuild_count() (a host counter): which of
    backward() and forward() still find what they need, and how many list builds the next forward() takes;
  * the frame of the next forward() and the gradients of the backward() behind it are, bit for bit, those of a FRESH
    context loaded with the same target, splats and moments (and held set): whatever the event left standing describes
    the current parameters.  Deterministic mode, so the gradients do not depend on the order the tiles arrive in, and no
    tolerance is involved.

The nudges of 0.25 px stay inside the 2-pixel margin the lists were built with (no build); the moves of 20 px leave it
(one build, asked for by the containment check of the projection that follows the event).
"""
import functools
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

S2D = importlib.import_module("2dgaussiansplatting_amd")
D = importlib.import_module("2dgaussiansplatting_amd.distributed")

W, H, N, RANK = 64, 48, 300, 1
KW = dict(deterministic=True, rebin_interval=1000)
E_STATE = 5
SLAB = dict(KW, row_begin=0, row_end=16)  # halo_commit: a context of the image's upper third, as held sets come with slabs


@functools.lru_cache(maxsize=None)
def scene():
    rng = np.random.default_rng(151)
    s = np.zeros(N, dtype=S2D.SPLAT_DTYPE)
    s["pos"][:, 0] = rng.uniform(4, W - 5, N)
    s["pos"][:, 1] = rng.uniform(4, H - 5, N)
    s["sx"] = rng.uniform(0.5, 0.9, N)
    s["sy"] = rng.uniform(0.5, 0.9, N)
    s["rot"] = rng.uniform(0, np.pi, N)
    s["color"] = rng.uniform(0, 1, (N, 3))
    s["opacity"] = rng.uniform(0.3, 0.9, N)
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def target(which=0):
    a = np.random.default_rng(7 + which).uniform(0, 1, (H, W, 4)).astype(np.float32)
    a.setflags(write=False)
    return a


def device_rows(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda().contiguous()


def mask_of(held):
    return device_rows(held.astype(np.int32) << RANK)


def refused(call):
    with pytest.raises(S2D.S2DError) as e:
        call()
    return e.value.code


def rows_f32(splats):
    return splats.view(np.float32).reshape(N, 9).copy()


def settle(t, want_builds, tgt=0, held=None, backwards_before=0, kw=KW):
    """forward() + backward() on the context the event happened to, and on a fresh one (created with kw) loaded with its
    state (held: the held set to commit there; backwards_before: backward passes the case already ran on the current
    parameters -- the gradient buffer adds passes up until an Adam step, so the fresh context runs as many).  want_builds: the list builds
    the forward() takes, a number or a tuple of admissible ones."""
    splats = t.get_splats()
    ad, b1, b2, it = t.get_adam()
    r0 = t.rebuild_count()
    t.forward()
    builds = t.rebuild_count() - r0
    t.backward()
    got = t.get_image().tobytes(), t.get_grads().tobytes()
    with S2D.Trainer(W, H, N, **kw) as f:
        f.set_target(target(tgt))
        f.set_splats(splats)
        f.set_adam(ad, b1, b2, it)
        if held is not None:
            D.HipHaloOps(f, N, "cuda").halo_commit(mask_of(held), RANK)
        for _ in range(backwards_before + 1):
            f.forward()
            f.backward()
        want = f.get_image().tobytes(), f.get_grads().tobytes()
    print("list builds of the forward after the event: %d (expected %r)" % (builds, want_builds))
    assert builds in (want_builds if isinstance(want_builds, tuple) else (want_builds,))
    assert got[0] == want[0], "image differs from a fresh context's"
    assert got[1] == want[1], "gradients differ from a fresh context's"


def nudged(t, rows, by):
    s = t.get_splats()
    s["pos"][rows, 0] += np.float32(by)
    return s


def far_row(t):
    """A row that can move 20 px to the right and stay inside the image."""
    return int(np.flatnonzero(t.get_splats()["pos"][:, 0] < W - 30)[0])


def case_set_target(t):
    t.set_target(target(1))
    assert refused(t.backward) == E_STATE       # the frame and the gradients were those of the old target
    settle(t, 0, tgt=1)


def case_set_splats_read_back(t):
    t.set_splats(t.get_splats())                # the same values: the call does not look
    assert refused(t.backward) == E_STATE
    settle(t, 1)


def case_init(t):
    t.init()
    assert refused(t.backward) == E_STATE
    settle(t, 1)


def scatter_splats(t, rows, by):
    s = rows_f32(nudged(t, rows, by))
    ids = np.asarray(rows, dtype=np.int32)
    D.HipHaloOps(t, N, "cuda").rows_scatter(D.ROWS_SPLATS, device_rows(ids), device_rows(s[ids]))
    assert refused(t.backward) == E_STATE


def case_rows_splats_nudged(t):
    scatter_splats(t, [3, 77, 150, 299], 0.25)
    settle(t, 0)


def case_rows_splats_moved(t):
    scatter_splats(t, [far_row(t)], 20.0)
    settle(t, 1)


def splats_from_device(t, rows, by):
    import torch
    d = device_rows(rows_f32(nudged(t, rows, by)))
    torch.cuda.synchronize()
    t.set_splats_device(d.data_ptr())
    t.synchronize()                             # (the copy is done before `d` goes)
    assert refused(t.backward) == E_STATE


def case_set_splats_device_nudged(t):
    splats_from_device(t, slice(None), 0.25)
    settle(t, 0)


def case_set_splats_device_moved(t):
    splats_from_device(t, slice(None), 0.25)
    splats_from_device(t, [far_row(t)], 20.0)
    settle(t, 1)


def case_rows_adam(t):
    rng = np.random.default_rng(5)
    ids = np.array([3, 77, 150, 299], dtype=np.int32)
    rows = rng.standard_normal((len(ids), 18)).astype(np.float32) * np.float32(1e-3)
    rows[:, 1::2] = np.abs(rows[:, 1::2])       # (m, v) pairs: a second moment is never negative
    D.HipHaloOps(t, N, "cuda").rows_scatter(D.ROWS_ADAM, device_rows(ids), device_rows(rows))
    t.backward()                                # what is drawn depends on the parameters only: the frame still stands
    settle(t, 0, backwards_before=1)


def case_set_adam(t):
    ad, b1, b2, it = t.get_adam()
    ad["mv"] *= np.float32(0.5)
    t.set_adam(ad, b1, b2, it)
    t.backward()
    settle(t, 0, backwards_before=1)


def case_rows_grads(t):
    ids = np.array([3, 77, 150], dtype=np.int32)
    rows = np.random.default_rng(6).standard_normal((len(ids), 9)).astype(np.float32)
    ops = D.HipHaloOps(t, N, "cuda")
    ops.rows_scatter(D.ROWS_GRADS, device_rows(ids), device_rows(rows))
    g = rows_f32(t.get_grads())
    assert g[ids].tobytes() == rows.tobytes()
    g[ids] = 0
    assert not g.any()                          # (the Adam step left every other record zero)
    ops.rows_scatter(D.ROWS_GRADS, device_rows(ids), device_rows(np.zeros_like(rows)))
    t.backward()                                # nothing is stale
    settle(t, 0, backwards_before=1)


def case_seed_ids(t):
    assert t.seed(ids=[5, 120, 240], seed=3) == 3
    assert refused(t.backward) == E_STATE
    settle(t, (0, 1))


def case_relocate(t):
    t.backward(density_stats=True)
    t.adam_step()
    t.forward()
    stats, passes = t.density()
    weight = np.sort(stats[:, 2].astype(np.float64) / passes)
    assert passes == 1 and weight[3] < weight[4]
    assert t.relocate(4, 0.5 * (weight[3] + weight[4])) == 4   # the four lowest weights are starved, everyone else may donate
    assert refused(t.backward) == E_STATE
    settle(t, (0, 1))


def zero_grads(ops):
    """(The gradient buffer adds backward passes up until an Adam step; a write of gradient rows makes nothing stale.)"""
    ops.rows_scatter(D.ROWS_GRADS, device_rows(np.arange(N, dtype=np.int32)), device_rows(np.zeros((N, 9), dtype=np.float32)))


def case_halo_commit(t):
    ops = D.HipHaloOps(t, N, "cuda")
    far = scene()["pos"][:, 1] > 32             # 16 rows and more below the slab: they reach none of its pixels
    first = (np.arange(N) % 2 == 0) | far
    assert far.sum() > 10 and not first.all()
    ops.halo_commit(mask_of(first), RANK)
    settle(t, 1, held=first, kw=SLAB)           # a first held set: the lists hold the held splats only
    fewer = first & ~far                        # departures alone, of splats that can no longer reach the slab
    zero_grads(ops)
    ops.halo_commit(mask_of(fewer), RANK, added=False)
    settle(t, 0, held=fewer, kw=SLAB)
    zero_grads(ops)
    t.halo_commit(None, RANK, 1)                # every splat again
    settle(t, 1, kw=SLAB)


def case_adam_step(t):
    t.backward()
    t.adam_step()
    assert refused(t.backward) == E_STATE
    settle(t, 0)                                # (steps of 0.05 px: the containment check asks for nothing)


CASES = {f.__name__[len("case_"):]: f for f in (
    case_set_target, case_set_splats_read_back, case_init, case_rows_splats_nudged, case_rows_splats_moved,
    case_set_splats_device_nudged, case_set_splats_device_moved, case_rows_adam, case_set_adam, case_rows_grads,
    case_seed_ids, case_relocate, case_halo_commit, case_adam_step)}


@pytest.mark.parametrize("event", sorted(CASES))
def test_event_leaves_what_a_fresh_context_has(event):
    with S2D.Trainer(W, H, N, **(SLAB if event == "halo_commit" else KW)) as t:
        t.set_target(target(0))
        t.set_splats(scene())
        t.forward()
        t.backward()
        t.adam_step()
        t.forward()
        assert t.rebuild_count() == 1            # the lists of the first forward are re-used
        CASES[event](t)
