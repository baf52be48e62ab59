#!/usr/bin/env python3
"""GPU-box tool: what the density statistics cost the separate backward pass -- s2d_backward with and without
S2D_BWD_DENSITY_STATS, float atomics and deterministic sums, on ONE box in ONE call, alternating, by the method of
tools/gpu_ab_backward.py: each figure is `iters` calls behind one s2d_forward of the same frame (4096^2 / 1 M after 30
iterations), every repetition is printed, so the spread of repeated runs is on the page next to the difference.
  python tools/gpu_ab_density.py [reps] [iters]"""
import importlib, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
S2D = importlib.import_module("2dgaussiansplatting_amd")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 100
W = H = 4096
N = 1_000_000


def run(deterministic, stats):
    with S2D.Trainer(W, H, N, deterministic=deterministic) as t:
        t.set_target_synthetic(); t.init()
        t.step(30, want_mse=False)
        t.forward()
        call = lambda: t.backward(skip_opacity_grad=False, density_stats=stats)  # noqa: E731
        for _ in range(5):
            call()
        t.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            call()
        t.synchronize()
        dt = time.perf_counter() - t0
    return 1e3 * dt / iters


rows = [("atomic        plain", False, False), ("atomic        statistics", False, True),
        ("deterministic plain", True, False), ("deterministic statistics", True, True)]
ms = {name: [] for name, _, _ in rows}
for r in range(reps):
    for name, det, stats in rows:
        ms[name].append(run(det, stats))
for name, _, _ in rows:
    v = ms[name]
    print("%-26s ms per call: %s   min %.4f  max %.4f  spread %.2f %%" % (name, " ".join("%.4f" % x for x in v), min(v), max(v),
                                                                     100.0 * (max(v) / min(v) - 1.0)), flush=True)
for k in (0, 2):
    a, b = min(ms[rows[k][0]]), min(ms[rows[k + 1][0]])
    print("%-26s best against the plain pass's best: %+.2f %%" % (rows[k + 1][0], 100.0 * (b / a - 1.0)))
