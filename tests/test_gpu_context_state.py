"""The context's two small state machines, pinned on bits through the C ABI.

  * Where a splat's parameters and moments live: with slab ownership the Adam step works on compact arrays of the held
    splats (S2D_COMPACT_HELD, default on), and the id-indexed arrays are brought up to date before anything else reads or
    writes them.  Every reader and writer is passed with the compact copy ahead of them, once with the copy and once
    without: no array read back may differ in a bit.
  * Who sums the squared error of a backward pass: the raster launch's last tile, the next Adam launch (one workgroup, or
    chunks shared between its first workgroups), or the standalone kernel.  Each of them adds the same tile errors in the
    same fixed order, so the double in the trace does not depend on the calls that led to it.
"""
import contextlib
import importlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

S2D = importlib.import_module("2dgaussiansplatting_amd")


@contextlib.contextmanager
def environment(name, value):
    """The library reads its switches when a context is created: set around Trainer(), as Trainer sets S2D_CHUNK_PAIRS."""
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        yield
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


def held_set_script(compact):
    """The fixed call sequence of test_compact_held_copy_changes_no_bit; returns every array read back, by name."""
    import torch
    D = importlib.import_module("2dgaussiansplatting_amd.distributed")
    W, H, n, rank = 64, 48, 700, 1
    rng = np.random.default_rng(11)
    out = {}

    def steps(t, k):
        for _ in range(k):
            t.forward_backward()
            t.adam_step()

    def mask_of(held):
        return torch.from_numpy(held.astype(np.int32) << rank).cuda().contiguous()

    with environment("S2D_COMPACT_HELD", "1" if compact else "0"):
        t = S2D.Trainer(W, H, n, deterministic=True)
    with t:
        t.set_target_synthetic()
        t.init()
        ops = D.HipHaloOps(t, n, "cuda")
        out["init"] = t.get_splats().view(np.float32).reshape(n, 9).copy()
        even = np.arange(n) % 2 == 0  # 350 held: one full Adam block of 256 and one of 94
        ops.halo_commit(mask_of(even), rank)
        steps(t, 3)                                                                      # 1
        out["splats_2"] = t.get_splats().view(np.float32).reshape(n, 9).copy()           # 2
        ids_g = torch.from_numpy(rng.permutation(n)[:50].astype(np.int32)).cuda()
        out["ids_g"] = ids_g.cpu().numpy()
        out["gather_3"] = ops.rows_gather(D.ROWS_SPLATS, ids_g).cpu().numpy()            # 3
        ids_s = rng.permutation(n)[:50].astype(np.int32)
        assert even[ids_s].any() and not even[ids_s].all()  # held and not held among them
        out["ids_s"] = ids_s
        out["rows_s"] = rng.standard_normal((50, 18)).astype(np.float32) * np.float32(1e-3)
        out["rows_s"][:, 1::2] = np.abs(out["rows_s"][:, 1::2])  # (m, v) pairs: a second moment is never negative
        ops.rows_scatter(D.ROWS_ADAM, torch.from_numpy(ids_s).cuda(), torch.from_numpy(out["rows_s"]).cuda())  # 4
        steps(t, 2)                                                                      # 5
        out["masks_6"] = ops.halo_masks([0, 16, 32, 48], 2.0).cpu().numpy()              # 6
        out["adam_7"] = t.get_adam()[0].view(np.float32).reshape(n, 18).copy()           # 7
        own = torch.from_numpy(t.get_splats().view(np.float32).reshape(n, 9).copy()).cuda()
        torch.cuda.synchronize()
        t.set_splats_device(own.data_ptr())                                              # 8: the context's own parameters
        t.synchronize()
        third = np.arange(n) % 3 == 0
        ops.halo_commit(mask_of(third), rank, added=True)                                # 9
        steps(t, 2)                                                                      # 10
        torch.cuda.synchronize()
        t.halo_commit(None, rank, 1)                                                     # 11: back to all held
        steps(t, 1)                                                                      # 12
        out["splats_13"] = t.get_splats().view(np.float32).reshape(n, 9).copy()          # 13
        out["adam_13"] = t.get_adam()[0].view(np.float32).reshape(n, 18).copy()
        out["trace_13"] = t.sqerr_trace(0, 8)
        t.synchronize()
    return out


def test_compact_held_copy_changes_no_bit():
    a, b = held_set_script(compact=False), held_set_script(compact=True)
    assert sorted(a) == sorted(b)
    for k in sorted(a):
        assert a[k].tobytes() == b[k].tobytes(), k
    for r in (a, b):
        n = len(r["init"])
        odd = np.arange(n) % 2 == 1
        # splats not held are unchanged by the steps in between, held ones moved
        assert r["splats_2"][odd].tobytes() == r["init"][odd].tobytes()
        assert (r["splats_2"][~odd] != r["init"][~odd]).any()
        # (nothing ran between the read-back and the gather: the same rows)
        assert r["gather_3"].tobytes() == r["splats_2"][r["ids_g"]].tobytes()
        # moments of the splats not held: what was scattered into them, zero elsewhere
        scattered = np.zeros(n, dtype=bool)
        scattered[r["ids_s"]] = True
        assert not r["adam_7"][odd & ~scattered].any()
        sel = odd[r["ids_s"]]
        assert r["adam_7"][r["ids_s"][sel]].tobytes() == r["rows_s"][sel].tobytes()
        assert r["adam_7"][~odd].any()
        assert np.isfinite(r["trace_13"]).all() and (r["trace_13"] > 0).all()
        assert (r["splats_13"] != r["splats_2"]).any()


# (W, H, splats): one scene per way of summing the tile errors when a whole iteration is queued
SUM_SCENES = {
    "in_raster": (64, 48, 300),            # 12 tiles, 2 Adam blocks: the raster launch's last tile
    "adam_one_workgroup": (64, 48, 16400),   # 65 Adam blocks >= 64 chunks, <= 1024 tiles: one workgroup of the Adam launch
    "adam_chunked": (528, 512, 16400),     # 33 x 32 = 1056 tiles > 1024: chunks shared by the Adam launch's workgroups
    "standalone": (528, 512, 300),         # too many tiles for the raster launch, too few blocks for Adam: the kernel of its own
}


@pytest.mark.parametrize("scene", sorted(SUM_SCENES))
def test_every_way_of_summing_the_squared_error_gives_the_same_double(scene):
    W, H, n = SUM_SCENES[scene]

    def route(calls):
        with S2D.Trainer(W, H, n) as t:
            t.set_target_synthetic()
            t.init()
            calls(t)
            v = t.sqerr_trace(0, 1)
            later = t.sqerr_trace(7, 1)
            t.synchronize()
            return v, later

    def two_passes(t):
        t.forward()
        t.backward()

    def fused_then_adam(t):
        t.forward_backward()
        t.adam_step()

    def fused_then_new_count(t):
        t.forward_backward()
        ad, b1, b2, _ = t.get_adam()
        t.set_adam(ad, b1, b2, 7)

    want, _ = route(two_passes)
    print("%s: squared error of iteration 0 = %r" % (scene, want[0]))
    assert np.isfinite(want[0]) and want[0] > 0
    routes = [("forward_backward", lambda t: t.forward_backward()), ("forward_backward; adam_step", fused_then_adam),
              ("step(1)", lambda t: t.step(1))]
    for name, calls in routes:
        got, _ = route(calls)
        print("  %-30s %r" % (name, got[0]))
        assert got.tobytes() == want.tobytes(), name
    if scene.startswith("adam"):
        # the sum was left to an Adam launch that never came: it lands in the slot of the pass's own iteration
        got, later = route(fused_then_new_count)
        print("  %-30s %r (slot 7: %r)" % ("forward_backward; set_adam(7)", got[0], later[0]))
        assert got.tobytes() == want.tobytes()
        assert later[0] == 0.0


def test_no_splats_still_has_an_mse():
    W, H = 64, 48
    ref = np.random.default_rng(3).uniform(0, 1, (H, W, 4)).astype(np.float32)
    with S2D.Trainer(W, H, 0) as t:
        t.set_target(ref)
        t.init()
        t.forward()
        t.backward()
        want = np.float64(t.mse())
    with S2D.Trainer(W, H, 0) as t:
        t.set_target(ref)
        t.init()
        got = t.step(2)
    print("mse without splats: step(2) = %r, forward; backward; mse() = %r" % (got.tolist(), float(want)))
    assert got[0].tobytes() == want.tobytes() and got[1].tobytes() == want.tobytes()
    # the framebuffer is black: float per pixel, double across pixels (main.cpp:801-805)
    e = ref[:, :, :3] * np.float32(255.0)
    per_pixel = (e[:, :, 0] * e[:, :, 0] + e[:, :, 1] * e[:, :, 1]) + e[:, :, 2] * e[:, :, 2]
    numpy_mse = per_pixel.astype(np.float64).sum() / (3.0 * W * H)
    assert abs(got[0] - numpy_mse) <= 1e-9 * numpy_mse and abs(want - numpy_mse) <= 1e-9 * numpy_mse
