"""CPU tests of importance-sampled placement (include/splat2d.h, s2d_importance / s2d_seed_splats / s2d_reseed).

tests/seed_ref.py restates the definitions in NumPy.  Here the restatement itself is checked -- its sampler against a
brute-force cumulative sum in Python integers, its pcg3d against the oracle's, its importance against a 3 x 3 image worked out
by hand -- and the shared arithmetic the kernels are made of (csrc/s2d_seed_math.h) and the starved-row selection of
s2d_reseed (density_starved, csrc/s2d_density.h), compiled by g++ into a shim of their own
(tests/hostcheck/s2d_seed_check.cpp), are held to it on bytes.  The entry points' argument checks run without a device.

This module is also where tests/test_gpu_seed.py takes the shim from.
"""
import ctypes as C
import importlib
import os
import subprocess
import tempfile

import numpy as np
import pytest

import oracle_lib as O
import seed_ref as R
import test_density_plan_cpu as DP

S2D = importlib.import_module("2dgaussiansplatting_amd")
CSRC = os.path.join(O.ROOT, "2dgaussiansplatting_amd", "csrc")
F32 = np.float32


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


_shim = None


def shim():
    global _shim
    if _shim is None:
        L = DP._shim("libs2d_seed_check.so", "s2d_seed_check.cpp",
                     [os.path.join(CSRC, h) for h in ("s2d_seed_math.h", "s2d_density.h", "s2d_math.h")])
        vp, i, u32, u64, f = C.c_void_p, C.c_int, C.c_uint32, C.c_uint64, C.c_float
        L.sc_importance.argtypes = [i, vp, vp, vp, i, i, i, u32, vp]
        L.sc_importance.restype = None
        L.sc_draws.argtypes = [vp, i, u32, u64, vp, vp]
        L.sc_draws.restype = None
        L.sc_rows.argtypes = [vp, vp, i, u32, u64, vp, i, i, i, f, f, vp]
        L.sc_rows.restype = None
        L.sc_starved.argtypes = [i, vp, i, i, f, vp]
        L.sc_starved.restype = i
        _shim = L
    return _shim


def shim_starved(stats, passes, max_moves, min_weight):
    st = np.ascontiguousarray(stats, dtype=F32).reshape(-1, 3)
    ids = np.full(max(min(int(max_moves), len(st)), 0) + 1, -1, dtype=np.int32)
    k = shim().sc_starved(len(st), _p(st), int(passes), int(max_moves), float(min_weight), _p(ids))
    assert 0 <= k < len(ids) and np.all(ids[k:] == -1)
    return ids[:k].copy()


def random_image(rng, H, W):
    img = rng.random((H, W, 4), dtype=F32)
    img[..., 3] = 1.0
    return img


# ---- the restatement itself ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(7, 5), (40, 1), (67, 61)])
def test_sampler_against_brute_force(W, H):
    rng = np.random.default_rng(W * 1000 + H)
    q = rng.integers(0, 8191, size=(H, W)).astype(np.uint32)
    q[rng.random((H, W)) < 0.3] = 0          # runs of zero importance must be stepped over
    q[0, 0] = 0
    total = sum(int(v) for v in q.reshape(-1))
    cum, run = [], 0
    for v in q.reshape(-1):
        run += int(v)
        cum.append(run)
    us = sorted(set([0, total - 1] + [c for c in cum if c < total] + [c - 1 for c in cum if c > 0] +
                    [int(v) for v in rng.integers(0, total, size=200)]))
    want = [next(p for p, c in enumerate(cum) if c > u) for u in us]
    got = R.sample(q, us)
    assert list(got) == want
    assert all(q.reshape(-1)[p] > 0 for p in got)
    # and the draws land in [0, total): (a * total) >> 64 with a < 2^64
    u, bx, by, az = R.draws(np.arange(500), 7, total)
    assert all(0 <= v < total for v in u)


def test_pcg3d_against_oracle():
    L = O.lib()
    rng = np.random.default_rng(1)
    cases = [(0, 0, 0), (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), (5, 2 * 3, R.STREAM), (5, 2 * 3 + 1, R.STREAM)]
    cases += [tuple(int(v) for v in rng.integers(0, 1 << 32, size=3)) for _ in range(200)]
    xs, ys, zs = R.pcg3d([c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases])
    for k, c in enumerate(cases):
        v = (C.c_uint32 * 3)(*c)
        L.s2do_pcg3d(v)
        assert (int(xs[k]), int(ys[k]), int(zs[k])) == tuple(v)


def test_importance_of_a_hand_computed_image():
    # 3 x 3, channels chosen so that every value below is exact in binary32
    ref = np.zeros((3, 3, 4), dtype=F32)
    ref[..., 0] = [[0.0, 0.25, 0.5], [0.0, 0.25, 0.5], [0.0, 0.25, 0.5]]   # a ramp along x
    ref[..., 1] = [[0.0, 0.0, 0.0], [0.125, 0.125, 0.125], [0.5, 0.5, 0.5]]  # steps along y
    ref[..., 2] = 0.75
    # edges: e_r = |r(x+1) - r(x-1)| clamped = .25, .5, .25 per column; e_g = |g(y+1) - g(y-1)| = .125, .5, .375 per row
    m = np.array([[0.375, 0.625, 0.375], [0.75, 1.0, 0.75], [0.625, 0.875, 0.625]])
    want = np.floor(np.minimum(1.0, m * 0.5) * 4095.0 + 0.5)
    # (the products are exact in double; binary32 rounds s * 4095 + 0.5 to within 2^-12 of them, far from an integer here)
    assert all(abs(v - round(v)) < 1e-9 or abs(v - round(v)) > 1e-3 for v in (np.minimum(1.0, m * 0.5) * 4095.0 + 0.5).reshape(-1))
    q, total = R.importance(R.EDGES, ref)
    assert q.tolist() == want.astype(int).tolist() and total == int(want.sum())
    q2, _ = R.importance(R.EDGES, ref, squared=True, floor=7)
    assert q2.tolist() == ((want.astype(np.int64) ** 2 >> 12) + 7).tolist()
    # error: image0 = ref + (.5, .25, -.75) on the centre pixel, ref elsewhere: m = 1.5 there -> s = min(1, 1.5 / 3)
    img = ref.copy()
    img[1, 1, :3] += F32([0.5, 0.25, -0.75])
    q, total = R.importance(R.ERROR, ref, image0=img)
    s = F32(1.5) * (F32(1.0) / F32(3.0))
    centre = int(s * F32(4095.0) + F32(0.5))
    assert centre in (2047, 2048) and total == centre and q[1, 1] == centre and np.count_nonzero(q) == 1
    img[0, 2, :3] = [1.0, 1.0, 0.0]  # |d| = .5 + 1 + .75 = 2.25 -> s = 0.75
    assert R.importance(R.ERROR, ref, image0=img)[0][0, 2] == int(F32(2.25) * (F32(1.0) / F32(3.0)) * F32(4095.0) + F32(0.5))
    img[2, 2, :3] = [2.0, 2.5, 0.5]  # |d| = 1.5 + 2 + .25 = 3.75 -> clamped to 1
    assert R.importance(R.ERROR, ref, image0=img)[0][2, 2] == 4095
    # caller: clamped to [0, 1], NaN -> 0
    plane = F32([[0.0, 0.5, 1.0], [2.0, -1.0, np.nan], [np.inf, -np.inf, 0.25]])
    q, total = R.importance(R.CALLER, caller=plane, floor=1)
    assert q.tolist() == [[1, 2049, 4096], [4096, 1, 1], [4096, 1, 1025]]
    assert total == int(q.sum())


# ---- the shared arithmetic and the selection, bytes-equal to the restatement ---------------------------------------------
@pytest.mark.parametrize("W,H", [(1, 1), (40, 1), (1, 9), (33, 17), (67, 61)])
def test_shim_importance_equals_restatement(W, H):
    rng = np.random.default_rng(W + 100 * H)
    ref, img = random_image(rng, H, W), random_image(rng, H, W)
    img[..., :3] = ref[..., :3] + (rng.random((H, W, 3), dtype=F32) - F32(0.5)) * F32(0.9)
    plane = (rng.random((H, W), dtype=F32) * F32(3.0) - F32(1.0)).astype(F32)
    plane.reshape(-1)[::5] = np.nan
    for source in (R.EDGES, R.ERROR, R.CALLER):
        for squared in (False, True):
            for floor in (0, 64):
                q = np.zeros((H, W), dtype=np.uint32)
                shim().sc_importance(source, _p(ref), _p(img), _p(plane), W, H, int(squared), floor, _p(q))
                want, _ = R.importance(source, ref, image0=img, caller=plane, squared=squared, floor=floor)
                assert q.tobytes() == want.tobytes(), (source, squared, floor)
    for mk in (R.round_fp16,):  # the images as a context with fp16 images holds them
        q = np.zeros((H, W), dtype=np.uint32)
        shim().sc_importance(R.ERROR, _p(mk(ref)), _p(mk(img)), None, W, H, 0, 0, _p(q))
        assert q.tobytes() == R.importance(R.ERROR, mk(ref), image0=mk(img))[0].tobytes()


@pytest.mark.parametrize("W,H,n", [(1, 1, 5), (40, 1, 64), (67, 61, 300)])
def test_shim_draws_and_rows_equal_restatement(W, H, n):
    rng = np.random.default_rng(W * H + n)
    ref = random_image(rng, H, W)
    ref[..., :3] = ref[..., :3] * F32(1.4) - F32(0.2)  # some channels outside [0, 1]: the colour is clamped
    q, total = R.importance(R.EDGES, ref, floor=3)
    ids = np.ascontiguousarray(rng.permutation(n)[: max(n // 2, 1)], dtype=np.int32)
    for seed in (0, 1, 0x7FFFFFFF, 0xFFFFFFFF):  # 2 * seed + 1 wraps mod 2^32
        u = np.zeros(len(ids), dtype=np.uint64)
        w3 = np.zeros((len(ids), 3), dtype=np.uint32)
        shim().sc_draws(_p(ids), len(ids), seed, total, _p(u), _p(w3))
        wu, bx, by, az = R.draws(ids, seed, total)
        assert [int(v) for v in u] == wu
        assert w3[:, 0].tobytes() == bx.tobytes() and w3[:, 1].tobytes() == by.tobytes() and w3[:, 2].tobytes() == az.tobytes()
        px = np.ascontiguousarray(R.sample(q, wu), dtype=np.int64)
        for scale, opacity in ((0.0, 0.0), (3.0, 0.5), (0.25, 1.0), (5000.0, 0.125)):
            out = np.zeros((len(ids), 9), dtype=F32)
            shim().sc_rows(_p(ids), _p(px), len(ids), seed, total, _p(ref), W, H, n, scale, opacity, _p(out))
            want = R.rows(ids, seed, q, total, ref, n, scale, opacity)
            assert out.tobytes() == want.tobytes(), (seed, scale, opacity)
            assert np.all(out[:, 0] <= W - 1) and np.all(out[:, 1] <= H - 1) and np.all(out[:, :2] >= 0)
    # the largest total the ABI can meet (8192^2 pixels of 8190) and the largest 64-bit draw stay below total
    big = 8192 * 8192 * 8190
    u = np.zeros(len(ids), dtype=np.uint64)
    shim().sc_draws(_p(ids), len(ids), 3, big, _p(u), _p(np.zeros((len(ids), 3), dtype=np.uint32)))
    assert [int(v) for v in u] == R.draws(ids, 3, big)[0] and all(int(v) < big for v in u)


def density_cases():
    rng = np.random.default_rng(11)
    n = 200
    st = np.zeros((n, 3), dtype=F32)
    st[:, :2] = rng.random((n, 2), dtype=F32) + F32(0.1)   # every splat could be a donor
    st[:, 2] = rng.random(n, dtype=F32) * F32(40.0)
    st[10:20, 2] = st[30:40, 2]                            # ties in w: the index decides
    st[50, 2] = np.nan                                     # never starved
    st[51, 2] = 0.0
    return n, st


@pytest.mark.parametrize("passes,max_moves,min_weight", [(1, 10, 5.0), (4, 1000, 5.0), (3, 7, float("inf")), (2, 0, 5.0), (5, 20, 0.0),
                                                         (1, 20, 1e-30)])
def test_starved_selection_equals_restatement(passes, max_moves, min_weight):
    n, st = density_cases()
    got = shim_starved(st, passes, max_moves, min_weight)
    want = R.starved(st, passes, max_moves, min_weight)
    assert got.tobytes() == want.tobytes()
    assert len(got) <= max_moves and 50 not in got
    assert len(shim_starved(st, 0, 10, 5.0)) == 0 and len(shim_starved(st[:0], 1, 10, 5.0)) == 0


def test_starved_selection_is_the_planners_when_donors_are_plentiful():
    n, st = density_cases()
    rng = np.random.default_rng(12)
    splats = rng.random((n, 9), dtype=F32) * F32(8.0) + F32(1.0)
    adams = np.zeros((n, 18), dtype=F32)
    for passes, max_moves, min_weight in ((1, 10, 5.0), (4, 60, 4.0), (2, 33, 10.0)):
        ids, _, _ = DP.plan(st, passes, max_moves, min_weight, 1.6, 256, 256, splats, adams)
        got = shim_starved(st, passes, max_moves, min_weight)
        assert len(ids) == len(got) > 0          # (no starved row was dropped for want of a donor)
        assert ids[:, 1].tolist() == got.tolist()


# ---- the boundary -------------------------------------------------------------------------------------------------------
def test_seed_config_layout_matches_header():
    code = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "splat2d.h"
    int main(void) {
        printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %u %u %u %u\n", sizeof(s2d_seed_config), offsetof(s2d_seed_config, struct_size),
               offsetof(s2d_seed_config, source), offsetof(s2d_seed_config, flags), offsetof(s2d_seed_config, seed),
               offsetof(s2d_seed_config, floor), offsetof(s2d_seed_config, scale), offsetof(s2d_seed_config, opacity),
               offsetof(s2d_seed_config, importance_device), S2D_SEED_TARGET_EDGES, S2D_SEED_ERROR, S2D_SEED_CALLER, S2D_SEED_SQUARED);
        return 0;
    }'''
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write(code)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(O.ROOT, "include"), src, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    T = S2D._SeedConfig
    assert got[0] == C.sizeof(T)
    assert got[1:9] == [T.struct_size.offset, T.source.offset, T.flags.offset, T.seed.offset, T.floor.offset, T.scale.offset,
                        T.opacity.offset, T.importance_device.offset]
    assert got[9:] == [S2D.S2D_SEED_TARGET_EDGES, S2D.S2D_SEED_ERROR, S2D.S2D_SEED_CALLER, S2D.S2D_SEED_SQUARED]
    assert (R.EDGES, R.ERROR, R.CALLER) == (S2D.S2D_SEED_TARGET_EDGES, S2D.S2D_SEED_ERROR, S2D.S2D_SEED_CALLER)


def bad_configs():
    """(what, field changes) of every configuration the three entry points refuse with S2D_E_INVALID."""
    return [("struct_size", dict(struct_size=8)), ("source", dict(source=3)), ("flags", dict(flags=2)), ("floor", dict(floor=4096)),
            ("negative scale", dict(scale=-1.0)), ("infinite scale", dict(scale=float("inf"))), ("NaN scale", dict(scale=float("nan"))),
            ("opacity > 1", dict(opacity=1.5)), ("opacity < 0", dict(opacity=-0.5)), ("NaN opacity", dict(opacity=float("nan"))),
            ("caller without a plane", dict(source=2)), ("a plane without caller", dict(importance_device=256))]


def good_config():
    return S2D._SeedConfig(C.sizeof(S2D._SeedConfig), 0, 0, 0, 0, 0.0, 0.0, None)


def test_entry_points_check_arguments_without_a_device():
    S2D._build.build_hip_library()
    L = S2D.load_library()
    cfg = good_config()
    total, placed = C.c_uint64(), C.c_int32()
    assert L.s2d_importance(None, C.byref(cfg), None, C.byref(total)) == 1
    assert L.s2d_seed_splats(None, C.byref(cfg), None, 0, C.byref(placed)) == 1
    assert L.s2d_reseed(None, C.byref(cfg), 1, C.c_float(1.0), C.byref(placed)) == 1
    # a context (where there is no device, the one s2d_create hands out for s2d_last_error): the configuration is judged
    # before any device work, and a good one then meets the missing target
    c = S2D._Config()
    c.struct_size = C.sizeof(S2D._Config)
    c.width, c.height, c.n_splats = 32, 16, 8
    h = C.c_void_p()
    rc = L.s2d_create(C.byref(c), C.byref(h))
    assert rc in (0, 2) and h.value
    try:
        assert L.s2d_importance(h, None, None, None) == 1
        assert L.s2d_seed_splats(h, None, None, 0, None) == 1
        assert L.s2d_reseed(h, None, 1, C.c_float(1.0), None) == 1
        for what, change in bad_configs():
            cfg = good_config()
            for k, v in change.items():
                setattr(cfg, k, v)
            assert L.s2d_importance(h, C.byref(cfg), None, C.byref(total)) == 1, what
            assert L.s2d_seed_splats(h, C.byref(cfg), None, 8, C.byref(placed)) == 1, what
            assert L.s2d_reseed(h, C.byref(cfg), 1, C.c_float(1.0), C.byref(placed)) == 1, what
            assert L.s2d_last_error(h)
        cfg = good_config()
        for ids in ([0, 8], [-1, 2], [3, 3]):
            a = np.array(ids, dtype=np.int32)
            assert L.s2d_seed_splats(h, C.byref(cfg), _p(a), len(a), None) == 1, ids
        assert L.s2d_seed_splats(h, C.byref(cfg), None, 9, None) == 1 and L.s2d_seed_splats(h, C.byref(cfg), None, -1, None) == 1
        assert L.s2d_reseed(h, C.byref(cfg), -1, C.c_float(1.0), None) == 1
        assert L.s2d_reseed(h, C.byref(cfg), 1, C.c_float(float("nan")), None) == 1
        # nothing wrong with the arguments: the call order is what is left to refuse (no target yet)
        assert L.s2d_importance(h, C.byref(cfg), None, C.byref(total)) == 5
        assert L.s2d_seed_splats(h, C.byref(cfg), None, 8, C.byref(placed)) == 5 and placed.value == 0
        assert L.s2d_reseed(h, C.byref(cfg), 1, C.c_float(1.0), C.byref(placed)) == 5
    finally:
        L.s2d_destroy(h)


def test_host_tool_refuses_what_it_cannot_combine():
    """--seed-init / --reseed-every with --gpus > 1, and the reseed options with --relocate-every (one owner of the statistics
    window): refused with a message before any device is touched."""
    S2D._build.build_hip_library()
    exe = S2D._build.build_host_program()
    base = [exe, "--synthetic", "64x48", "--splats", "50", "--iters", "4"]
    for extra, word in ((["--seed-init", "edges", "--gpus", "2"], "one context"), (["--reseed-every", "2", "--gpus", "2"], "one context"),
                        (["--reseed-every", "2", "--relocate-every", "2"], "choose one"), (["--seed-init", "corners"], "usage"),
                        (["--reseed-every", "2", "--reseed-window", "0"], "usage"), (["--reseed-every", "2", "--reseed-scale", "-1"], "usage")):
        r = subprocess.run(base + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
        assert r.returncode == 2 and word in r.stderr and not r.stdout, (extra, r.returncode, r.stderr[:200])
