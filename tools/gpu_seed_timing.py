#!/usr/bin/env python3
"""GPU-box tool: what importance-sampled placement costs beside one training iteration -- s2d_seed_splats over all rows and
one s2d_reseed at 4096^2 / 1 M splats, by the method of tools/gpu_ab_density.py: every figure is the wall time of `reps` calls
between two synchronisations, each repetition printed.  Both calls end with the host reading the map's total, so the wall time
of a call is its whole cost; the map alone (s2d_importance without the copy of q) is timed beside them.
  python tools/gpu_seed_timing.py [reps]"""
import ctypes as C
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
S2D = importlib.import_module("2dgaussiansplatting_amd")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
W = H = 4096
N = 1_000_000


def timed(t, call, prepare=None):
    out = []
    for _ in range(reps):
        if prepare:
            prepare()
        t.synchronize()
        t0 = time.perf_counter()
        call()
        t.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return out


def line(name, v):
    print("%-44s ms: %s   min %.3f  max %.3f" % (name, " ".join("%.3f" % x for x in v), min(v), max(v)), flush=True)


with S2D.Trainer(W, H, N) as t:
    t.set_target_synthetic()
    t.init()
    t.step(30, want_mse=False)
    t.synchronize()
    t0 = time.perf_counter()
    t.step(20, want_mse=False)
    t.synchronize()
    print("%-44s ms: %.3f" % ("one iteration (s2d_step, mean of 20)", 1e3 * (time.perf_counter() - t0) / 20), flush=True)
    t.forward()
    cfg = t._seed_config("error", True, 0, 3.0, 0.0, 1, None)
    total = C.c_uint64()
    line("map alone (s2d_importance, error, no copy)", timed(t, lambda: t._ck(t.L.s2d_importance(t._h, C.byref(cfg), None, C.byref(total)))))

    def stats_pass():
        t.step(1, want_mse=False, density_stats=True)
        t.forward()

    moved = []
    line("s2d_reseed (error, squared, 5 %% of %d)" % N, timed(t, lambda: moved.append(t.reseed(N // 20, float("inf"), source="error", squared=True,
                                                                                           scale=3.0, seed=len(moved))), stats_pass))
    print("  rows written per call: %s" % moved)
    line("s2d_seed_splats, all rows (edges, floor 64)", timed(t, lambda: t.seed(source="edges", floor=64, seed=2)))
    line("s2d_seed_splats, all rows (error, squared)", timed(t, lambda: t.seed(source="error", squared=True, seed=3), t.forward))
    t.step(5, want_mse=False)   # (the context goes on: lists and projection follow the new rows)
    t.synchronize()
