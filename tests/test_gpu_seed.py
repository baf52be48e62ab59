"""GPU tests of importance-sampled placement: s2d_importance, s2d_seed_splats, s2d_reseed (include/splat2d.h).

The yardstick is tests/seed_ref.py, a NumPy restatement of the header's definitions that tests/test_seed_cpu.py checks on its
own; the device is held to it on BYTES -- the map, its total, and every row written.  Shapes are chosen for the share / scan /
search structure of csrc/s2d_seed.hip (shares of 1024 consecutive pixels, chunks of 64, one scan workgroup of 256 threads):
1 x 1; 40 x 1 (less than a chunk); 33 x 17 (less than a share); 67 x 61 (four shares, the last ragged); the squirrel mini
268 x 213; 640 x 410 (257 shares: more than the scan workgroup has threads, the last a share of 256 pixels).

The training test takes its bar from the ORACLE's run of the same schedule (tools/seed_oracle_schedule.py), not from the code
under test: see test_reseeding_lowers_the_final_error.
"""
import functools
import importlib
import os

import numpy as np
import pytest

import oracle_lib as O
import seed_ref as R
import test_seed_cpu as SC

pytestmark = pytest.mark.gpu

S2D = importlib.import_module("2dgaussiansplatting_amd")
MINI = os.path.join(O.GOLDEN, "squirrel_cls_mini_268x213.s2di")
F32 = np.float32
SHAPES = {"1x1": (1, 1, 5), "40x1": (40, 1, 30), "33x17": (33, 17, 200), "67x61": (67, 61, 300), "mini": (268, 213, 1024),
          "640x410": (640, 410, 2000)}
SOURCES = ("edges", "error", "caller")
SRC = {"edges": R.EDGES, "error": R.ERROR, "caller": R.CALLER}


@functools.lru_cache(maxsize=None)
def target(name):
    """The squirrel mini, or smooth blobs under noise (edges of every strength) in [0, 1]."""
    if name == "mini":
        return O.target_rgba32f(O.load_s2di(MINI))
    W, H, _ = SHAPES[name]
    rng = np.random.default_rng(W * 7 + H)
    y, x = np.mgrid[0:H, 0:W].astype(F32)
    img = np.zeros((H, W, 4), dtype=F32)
    for c in range(3):
        img[..., c] = 0.5 + 0.35 * np.sin(x * F32(0.21 + 0.05 * c) + y * F32(0.13)) + 0.15 * (rng.random((H, W), dtype=F32) - 0.5)
    img[..., :3] = np.clip(img[..., :3], 0.0, 1.0)
    img[H // 2:, W // 2:, :3] = img[H // 2, W // 2, :3]  # a flat quarter: runs of zero importance
    img[..., 3] = 1.0
    return img


@functools.lru_cache(maxsize=None)
def caller_plane(name):
    W, H, _ = SHAPES[name]
    rng = np.random.default_rng(W + 31 * H)
    v = (rng.random((H, W), dtype=F32) * F32(1.6) - F32(0.3)).astype(F32)   # below 0 and above 1 as well
    v.reshape(-1)[::7] = np.nan
    v.reshape(-1)[3::11] = 0.0
    return v


def device_plane(v):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(v, dtype=F32)).cuda()
    torch.cuda.synchronize()
    return d


def trainer(name, fp16=False, steps=0, **kw):
    W, H, n = SHAPES[name]
    t = S2D.Trainer(W, H, n, fp16_images=fp16, **kw)
    t.set_target(target(name))
    t.init()
    if steps:
        t.step(steps)
    return t


def held_target(name, fp16):
    return R.round_fp16(target(name)) if fp16 else target(name)


def reference_map(t, name, fp16, source, squared=False, floor=0, plane=None):
    """-> (q, total) of the restatement on the images as the context holds them (image0 as s2d_get_image returns it)."""
    img = t.get_image() if source == "error" else None
    return R.importance(SRC[source], held_target(name, fp16), image0=img, caller=plane, squared=squared, floor=floor)


def _code(f):
    try:
        f()
    except S2D.S2DError as e:
        return e.code
    return 0


# ---------------------------------------------------------------------------------------------
# 1. the map
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_importance_equals_the_restatement(name, fp16):
    plane = caller_plane(name)
    d = device_plane(plane)
    with trainer(name, fp16=fp16, steps=5) as t:
        t.forward()                                 # ERROR is taken after 5 steps
        for source in SOURCES:
            for squared in (False, True):
                for floor in (0, 64):
                    ptr = d.data_ptr() if source == "caller" else None
                    q, total = t.importance(source, squared=squared, floor=floor, importance_ptr=ptr)
                    want, wtotal = reference_map(t, name, fp16, source, squared, floor, plane)
                    assert q.tobytes() == want.tobytes(), (source, squared, floor, int((q != want).sum()))
                    assert total == wtotal, (source, squared, floor)
        q, total = t.importance("edges")
        assert name == "1x1" or total > 0            # (a 1 x 1 image has no edge)


# ---------------------------------------------------------------------------------------------
# 2. placement
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_seeding_all_rows_equals_the_restatement(name, fp16):
    W, H, n = SHAPES[name]
    plane = caller_plane(name)
    d = device_plane(plane)
    with trainer(name, fp16=fp16, steps=5) as t:
        for k, source in enumerate(SOURCES):
            t.forward()
            squared, floor, scale, opacity, seed = (k == 1), (1 if name == "1x1" else 2 * k), (0.0, 3.0, 0.5)[k], (0.0, 0.75, 1.0)[k], 17 + k
            ptr = d.data_ptr() if source == "caller" else None
            q, total = reference_map(t, name, fp16, source, squared, floor, plane)
            assert total > 0
            placed = t.seed(source=source, squared=squared, floor=floor, scale=scale, opacity=opacity, seed=seed, importance_ptr=ptr)
            want = R.rows(np.arange(n), seed, q, total, held_target(name, fp16), n, scale, opacity)
            assert placed == n
            got = t.get_splats().view(F32).reshape(n, 9)
            assert got.tobytes() == want.tobytes(), (source, int((got != want).any(axis=1).sum()))
            assert not t.get_adam()[0].view(F32).any()


@pytest.mark.parametrize("name", ["40x1", "67x61", "640x410"])
def test_a_subset_writes_exactly_those_rows_of_the_full_call(name):
    W, H, n = SHAPES[name]
    rng = np.random.default_rng(n)
    ids = rng.permutation(n)[: n // 3].astype(np.int32)
    kw = dict(source="edges", floor=1, scale=2.5, opacity=0.5, seed=0xFFFFFFFF)
    with trainer(name, steps=5) as full:
        full.seed(**kw)
        want = full.get_splats().view(F32).reshape(n, 9)
    with trainer(name, steps=5) as t:
        s0, (a0, b1, b2, it) = t.get_splats().view(F32).reshape(n, 9).copy(), t.get_adam()
        a0 = a0.view(F32).reshape(n, 18).copy()
        assert a0.any() and it == 5
        assert t.seed(ids=ids, **kw) == len(ids)
        s1, (a1, c1, c2, it1) = t.get_splats().view(F32).reshape(n, 9), t.get_adam()
        a1 = a1.view(F32).reshape(n, 18)
        rest = np.setdiff1d(np.arange(n), ids)
        assert s1[ids].tobytes() == want[ids].tobytes()
        assert s1[rest].tobytes() == s0[rest].tobytes() and a1[rest].tobytes() == a0[rest].tobytes()
        assert not a1[ids].any()
        assert (c1, c2, it1) == (b1, b2, it)                      # beta1t, beta2t, iterations untouched
        # count rows without ids: rows 0 .. count - 1
        assert t.seed(count=7 if n >= 7 else n, **kw) == min(7, n)
        assert t.get_splats().view(F32).reshape(n, 9)[:min(7, n)].tobytes() == want[:min(7, n)].tobytes()


@pytest.mark.parametrize("name", ["67x61", "640x410"])
def test_one_hot_maps_land_every_row_in_their_pixel(name):
    W, H, n = SHAPES[name]
    last = W * H - 1
    tgt = target(name)
    with trainer(name) as t:
        for hot in ([0], [last], [1023, 1024], [last - 256, last] if name == "640x410" else [63, 64]):
            plane = np.zeros(W * H, dtype=F32)
            plane[hot] = 1.0
            d = device_plane(plane)
            q, total = t.importance("caller", importance_ptr=d.data_ptr())
            assert total == 4095 * len(hot) and np.flatnonzero(q.reshape(-1)).tolist() == hot
            assert t.seed(source="caller", seed=3, scale=1.0, importance_ptr=d.data_ptr()) == n
            got = t.get_splats().view(F32).reshape(n, 9)
            want = R.rows(np.arange(n), 3, q, total, tgt, n, 1.0, 0.0)
            assert got.tobytes() == want.tobytes(), hot
            # pos = pixel + a fraction in [0, 1], clamped to the image: the row's pixel is one of the hot ones
            px = np.minimum(np.floor(got[:, 1]), H - 1).astype(np.int64) * W + np.minimum(np.floor(got[:, 0]), W - 1).astype(np.int64)
            assert set(px.tolist()) == set(hot), hot


@pytest.mark.parametrize("name", ["33x17", "67x61"])
def test_an_all_zero_map_places_nothing_and_floor_one_is_uniform(name):
    W, H, n = SHAPES[name]
    d = device_plane(np.zeros((H, W), dtype=F32))
    with trainer(name, steps=5) as t:
        s0, a0 = t.get_splats().tobytes(), t.get_adam()[0].tobytes()
        q, total = t.importance("caller", importance_ptr=d.data_ptr())
        assert total == 0 and not q.any()
        assert t.seed(source="caller", importance_ptr=d.data_ptr()) == 0
        assert t.get_splats().tobytes() == s0 and t.get_adam()[0].tobytes() == a0
        t.step(1)                                                   # ... and the context goes on as if nothing had been asked
        q, total = t.importance("caller", floor=1, importance_ptr=d.data_ptr())
        assert total == W * H and (q == 1).all()
        assert t.seed(source="caller", floor=1, seed=9, importance_ptr=d.data_ptr()) == n
        want = R.rows(np.arange(n), 9, q, total, target(name), n, 0.0, 0.0)
        assert t.get_splats().view(F32).reshape(n, 9).tobytes() == want.tobytes()


# ---------------------------------------------------------------------------------------------
# 3. after a write
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("subset", [False, True], ids=["all", "subset"])
@pytest.mark.parametrize("name", ["67x61", "mini"])
def test_the_frame_after_a_write_is_that_of_a_fresh_context(name, subset):
    W, H, n = SHAPES[name]
    ids = np.arange(0, n, 3, dtype=np.int32) if subset else None
    with trainer(name, steps=5, deterministic=True) as t:           # lists and projection of the OLD parameters exist
        t.forward()
        t.seed(ids=ids, source="error", squared=True, scale=4.0, seed=5)
        written = np.arange(n) if ids is None else ids
        assert not t.get_adam()[0].view(F32).reshape(n, 18)[written].any()
        t.forward()
        img = t.get_image()
        splats = t.get_splats()
        with S2D.Trainer(W, H, n, deterministic=True) as fresh:
            fresh.set_target(target(name))
            fresh.set_splats(splats)
            fresh.forward()
            assert fresh.get_image().tobytes() == img.tobytes()
        mse = t.step(50)
        assert np.isfinite(mse).all()
        assert np.isfinite(t.get_splats().view(F32)).all() and np.isfinite(t.get_adam()[0].view(F32)).all()


# ---------------------------------------------------------------------------------------------
# 4. s2d_reseed
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,max_moves,min_weight", [("mini", 102, 5.0), ("mini", 5, float("inf")), ("67x61", 1000, 2.0), ("33x17", 0, 5.0)])
def test_reseed_writes_the_starved_rows(name, max_moves, min_weight):
    W, H, n = SHAPES[name]
    with trainer(name, steps=20, deterministic=True) as t:
        t.step(2, density_stats=True)
        t.forward()
        stats, passes = t.density()
        assert passes == 2
        ids = R.starved(stats, passes, max_moves, min_weight)
        assert ids.tobytes() == SC.shim_starved(stats, passes, max_moves, min_weight).tobytes()
        q, total = reference_map(t, name, False, "error", True, 0)
        s0, (a0, b1, b2, it) = t.get_splats().view(F32).reshape(n, 9).copy(), t.get_adam()
        a0 = a0.view(F32).reshape(n, 18).copy()
        moved = t.reseed(max_moves, min_weight, source="error", squared=True, floor=0, scale=3.0, seed=4)
        print("%s: %d of %d rows starved below %g" % (name, moved, n, min_weight))
        assert moved == len(ids) and (moved > 0 or max_moves == 0 or min_weight != float("inf"))
        s1, (a1, c1, c2, it1) = t.get_splats().view(F32).reshape(n, 9), t.get_adam()
        a1 = a1.view(F32).reshape(n, 18)
        rest = np.setdiff1d(np.arange(n), ids)
        assert s1[rest].tobytes() == s0[rest].tobytes() and a1[rest].tobytes() == a0[rest].tobytes()
        if len(ids):
            assert s1[ids].tobytes() == R.rows(ids, 4, q, total, target(name), n, 3.0, 0.0).tobytes()
            assert (s1[ids] != s0[ids]).any(axis=1).all()             # every one of them was written
            assert not a1[ids].any()
        assert (c1, c2, it1) == (b1, b2, it)
        d1, passes1 = t.density()
        assert passes1 == 0 and not d1.any()
        assert np.isfinite(t.step(5)).all()


# ---------------------------------------------------------------------------------------------
# 5. statuses
# ---------------------------------------------------------------------------------------------
def test_status_codes():
    import ctypes as C
    import torch
    name = "67x61"
    W, H, n = SHAPES[name]
    d = device_plane(np.ones((H, W), dtype=F32))
    total, placed = C.c_uint64(), C.c_int32()

    def three(t, cfg):
        return (t.L.s2d_importance(t._h, C.byref(cfg), None, C.byref(total)), t.L.s2d_seed_splats(t._h, C.byref(cfg), None, n, C.byref(placed)),
                t.L.s2d_reseed(t._h, C.byref(cfg), 5, C.c_float(1.0), C.byref(placed)))

    with trainer(name, steps=2) as t:
        t.step(1, density_stats=True)
        t.forward()
        before = t.get_splats().tobytes()
        for what, change in SC.bad_configs():                                      # S2D_E_INVALID, whatever the state
            cfg = SC.good_config()
            for k, v in change.items():
                setattr(cfg, k, d.data_ptr() if k == "importance_device" else v)
            assert three(t, cfg) == (1, 1, 1), what
        cfg = SC.good_config()
        for ids in ([0, n], [-1, 2], [3, 3]):
            a = np.array(ids, dtype=np.int32)
            assert t.L.s2d_seed_splats(t._h, C.byref(cfg), a.ctypes.data_as(C.c_void_p), len(a), None) == 1, ids
        assert t.L.s2d_seed_splats(t._h, C.byref(cfg), None, n + 1, None) == 1
        assert t.L.s2d_reseed(t._h, C.byref(cfg), -1, C.c_float(1.0), None) == 1
        assert t.L.s2d_reseed(t._h, C.byref(cfg), 1, C.c_float(float("nan")), None) == 1
        assert t.get_splats().tobytes() == before and t.density()[1] == 1          # nothing was written, nothing reset
        assert t.reseed(5, 1.0, source="edges") >= 0 and t.density()[1] == 0       # (the same arguments, accepted)
        assert _code(lambda: t.reseed(5, 1.0, source="edges")) == 5               # no statistics pass since the reset
        t.step(1)
        assert _code(lambda: t.importance("error")) == 5                           # no forward on the current parameters
        assert _code(lambda: t.seed(source="error")) == 5
        t.step(1, density_stats=True)
        assert _code(lambda: t.reseed(5, 1.0, source="error")) == 5
        assert t.density()[1] == 1
        t.forward()
        assert t.reseed(5, 1.0, source="error") >= 0
    with S2D.Trainer(W, H, n) as t:                                                 # no target
        t.init()
        assert _code(lambda: t.importance("edges")) == 5
        assert _code(lambda: t.seed(source="caller", importance_ptr=d.data_ptr())) == 5
        assert _code(lambda: t.reseed(5, 1.0, source="edges")) == 5
    with S2D.Trainer(W, 64, n, row_begin=16, row_end=48) as t:                      # a slab context
        t.set_target(np.ones((64, W, 4), dtype=F32))
        t.init()
        assert _code(lambda: t.importance("edges")) == 1
        assert _code(lambda: t.seed(source="edges")) == 1
        assert _code(lambda: t.reseed(5, 1.0, source="edges")) == 1
    with trainer(name) as t:                                                        # a context with a held set
        masks = torch.ones(t.n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        t.halo_commit(masks.data_ptr(), 0, 1)
        t.forward()
        t.backward(density_stats=True)
        assert _code(lambda: t.importance("edges")) == 1
        assert _code(lambda: t.seed(source="edges")) == 1
        assert _code(lambda: t.reseed(5, 1.0, source="edges")) == 1
    with trainer(name, reference_order=True) as t:                                  # where s2d_relocate refuses: no statistics
        t.forward()
        assert _code(lambda: t.reseed(5, 1.0, source="edges")) == 1
        assert t.seed(source="edges") == n                                          # (placement itself needs none)


# ---------------------------------------------------------------------------------------------
# 6. what it is for
# ---------------------------------------------------------------------------------------------
# tools/seed_oracle_schedule.py, the ORACLE's final MSEs of this schedule (300 iterations, one thread: the reference's order of sums):
ORACLE_PLAIN, ORACLE_RESEEDED = 84.7616, 76.9682
GAIN_BAR = 1.0 - 0.5 * (1.0 - ORACLE_RESEEDED / ORACLE_PLAIN)


def test_reseeding_lowers_the_final_error():
    """The squirrel mini, 1024 splats, deterministic sums, 300 iterations; before iterations 50, 100, ..., 250 the preceding
    iteration gathers the statistics, then forward() and reseed(102, 5.0) from the squared error map at scale 3 with seed
    k = iteration / 50.  The bar is half the ORACLE's relative gain on the same schedule: the two trajectories differ in the
    order of their sums only, and half the gain leaves more than twice the oracle's seed-to-seed spread (0.901 - 0.918) for
    that."""
    finals = {}
    for reseed in (False, True):
        with trainer("mini", deterministic=True) as t:
            mse = []
            for k in range(6):
                if k == 5 or not reseed:
                    mse += list(t.step(50))
                    continue
                mse += list(t.step(49))
                mse += list(t.step(1, density_stats=True))
                t.forward()
                moved = t.reseed(102, 5.0, source="error", squared=True, floor=0, scale=3.0, seed=k + 1)
                print("before iteration %d: %d rows reseeded (mse %.3f)" % (50 * (k + 1), moved, mse[-1]))
            assert len(mse) == 300 and np.isfinite(mse).all()
            finals[reseed] = mse[-1]
    ratio = finals[True] / finals[False]
    print("plain %.4f  reseeded %.4f  ratio %.4f  (oracle %.4f / %.4f = %.4f, bar %.4f)" %
          (finals[False], finals[True], ratio, ORACLE_PLAIN, ORACLE_RESEEDED, ORACLE_RESEEDED / ORACLE_PLAIN, GAIN_BAR))
    assert ratio <= GAIN_BAR, (ratio, GAIN_BAR)


def test_host_tool_seeds_and_reseeds():
    import re
    import subprocess
    exe = S2D._build.TRAIN_BIN
    base = [exe, "--image", MINI, "--splats", "1024", "--iters", "45", "--deterministic"]

    def run(extra):
        r = subprocess.run(base + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
        assert r.returncode == 0, r.stderr
        mse = [float(m) for m in re.findall(r"^\d+ itr, mse ([0-9.]+)$", r.stdout, flags=re.M)]
        assert len(mse) == 45 and np.isfinite(mse).all()
        return mse, r.stderr

    plain, _ = run([])
    seeded, err = run(["--seed-init", "edges"])
    assert "seeded 1024 splats from the target (edges)" in err
    assert abs(plain[0] - 5934.9042) < 1e-3 and seeded[0] < 0.5 * plain[0]      # a start that carries the target's colours
    reseeded, err = run(["--reseed-every", "20", "--reseed-window", "3", "--reseed-min-weight", "1e30"])
    assert re.findall(r"reseeded (\d+) splats before iteration (\d+)", err) == [("102", "20"), ("102", "40")]
    assert reseeded[:20] == plain[:20] and reseeded[21:] != plain[21:]           # the statistics passes change no result
