#!/usr/bin/env python3
"""GPU-box tool: what an alive set costs s2d_step -- on ONE box in ONE call, alternating, by the method of
tools/gpu_ab_density.py: each figure is `iters` iterations of s2d_step after `warmup` iterations at 4096^2, every repetition
is printed, so the spread of repeated runs is on the page next to the differences.
  (a) no set                         1 M rows
  (b) an all-ones set                1 M rows: the cost of the compact Adam path alone, (b) against (a)
  (c) every second row dead          1 M rows
  (d) rows [0, 500 000) dead         1 M rows
  (e) a context of 500 000 rows holding the alive rows of (d): what a dead row costs, (d) against (e)
Contexts are created one after another (each holds its own pair buffers); (e) starts from the rows (d) starts from.
  python tools/gpu_ab_alive.py [reps] [iters] [warmup] [json_out]"""
import importlib, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
S2D = importlib.import_module("2dgaussiansplatting_amd")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 100
warmup = int(sys.argv[3]) if len(sys.argv) > 3 else 200
json_out = sys.argv[4] if len(sys.argv) > 4 else None
W = H = 4096
N = 1_000_000


def mask_of(kind):
    if kind == "ones":
        return np.ones(N, dtype=np.uint8)
    m = np.zeros(N, dtype=np.uint8)
    if kind == "second":
        m[::2] = 1
    else:
        m[N // 2:] = 1
    return m


def run(kind):
    n = N // 2 if kind == "compact" else N
    with S2D.Trainer(W, H, n) as t:
        t.set_target_synthetic()
        if kind == "compact":       # the rows [N / 2, N) of init() over N rows
            with S2D.Trainer(W, H, N) as full:
                full.init()
                rows = full.get_splats()[N // 2:].copy()
            t.set_splats(rows)
        else:
            t.init()
        if kind not in ("none", "compact"):
            t.set_alive(mask_of(kind))
        t.step(warmup, want_mse=False)
        t.synchronize()
        t0 = time.perf_counter()
        t.step(iters, want_mse=False)
        t.synchronize()
        dt = time.perf_counter() - t0
        alive = t.alive()[1]
    return 1e3 * dt / iters, alive


rows = [("(a) no set", "none"), ("(b) all-ones set", "ones"), ("(c) every second dead", "second"), ("(d) first half dead", "half"),
        ("(e) 500 000 compact", "compact")]
ms = {name: [] for name, _ in rows}
alive = {}
for r in range(reps):
    for name, kind in rows:
        v, alive[name] = run(kind)
        ms[name].append(v)
for name, _ in rows:
    v = ms[name]
    print("%-24s %7d alive  ms per iteration: %s   min %.4f  max %.4f  spread %.2f %%"
          % (name, alive[name], " ".join("%.4f" % x for x in v), min(v), max(v), 100.0 * (max(v) / min(v) - 1.0)), flush=True)
best = {name: min(v) for name, v in ms.items()}
print("having a set, (b) against (a), best against best: %+.2f %%" % (100.0 * (best[rows[1][0]] / best[rows[0][0]] - 1.0)))
print("a dead row,   (d) against (e), best against best: %+.2f %%" % (100.0 * (best[rows[3][0]] / best[rows[4][0]] - 1.0)))
if json_out:
    with open(json_out, "w") as f:
        json.dump({"width": W, "height": H, "rows": N, "reps": reps, "iters": iters, "warmup": warmup,
                   "ms_per_iteration": ms, "alive": alive}, f, indent=1)
