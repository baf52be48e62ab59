#!/usr/bin/env python3
"""GPU-box tool: what the optimiser controls cost, by the method of tools/gpu_seed_timing.py: every figure
is the wall time of one call between two synchronisations, each repetition printed.

  python tools/gpu_optim_timing.py [reps]            s2d_adam_step at 4096^2 / 1 M after 30 iterations, alternating in one
      process between the plain launch (adam_kernel: the yardstick -- the parent's instructions), the second instantiation
      with rates equal to the default, and the second instantiation with 10 % of the rows frozen.  Every timed step follows
      an untimed forward + backward pass, so that it works on real gradients.
  python tools/gpu_optim_timing.py rebuilds          tile-list rebuilds (s2d_get_rebuild_count) per 100 iterations for the
      position rates 0.05 and 0.5 at rebin_margin 2 (the default) and at 2.35 * rate * 4: the squirrel mini / 1024 over 300
      iterations, and 4096^2 / 1 M over 100 iterations with the wall time per iteration."""
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
S2D = importlib.import_module("2dgaussiansplatting_amd")


def adam_timing(reps):
    W = H = 4096
    N = 1_000_000
    frozen = np.random.default_rng(1).random(N) < 0.1
    variants = [("plain launch (adam_kernel)", lambda t: (t.set_optim(None), t.set_frozen(None))),
                ("controls, five rates = training_rate", lambda t: (t.set_optim(), t.set_frozen(None))),
                ("controls, equal rates, 10 % frozen", lambda t: (t.set_optim(), t.set_frozen(frozen)))]
    times = {name: [] for name, _ in variants}
    with S2D.Trainer(W, H, N) as t:
        t.set_target_synthetic()
        t.init()
        t.step(30, want_mse=False)
        t.synchronize()
        for _ in range(reps):
            for name, select in variants:      # alternating: every variant sees the same drift of the run
                select(t)
                t.forward_backward(skip_image=True)
                t.synchronize()
                t0 = time.perf_counter()
                t.adam_step()
                t.synchronize()
                times[name].append(1e3 * (time.perf_counter() - t0))
    for name, _ in variants:
        v = times[name]
        print("%-40s ms: %s   min %.3f  max %.3f" % (name, " ".join("%.3f" % x for x in v), min(v), max(v)), flush=True)


def rebuilds():
    import oracle_lib as O
    mini = O.target_rgba32f(O.load_s2di(os.path.join(O.GOLDEN, "squirrel_cls_mini_268x213.s2di")))
    for scene, (W, H, N, iters) in (("mini 268x213 / 1024", (268, 213, 1024, 300)), ("4096^2 / 1 M", (4096, 4096, 1_000_000, 100))):
        for rate in (0.05, 0.5):
            for margin in (2.0, 2.35 * rate * 4):
                with S2D.Trainer(W, H, N, rebin_margin=margin) as t:
                    if N == 1024:
                        t.set_target(mini)
                    else:
                        t.set_target_synthetic()
                    t.init()
                    t.set_optim(pos=rate)
                    counts, before = [], t.rebuild_count()
                    t.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(iters // 100):
                        t.step(100, want_mse=False)
                        t.synchronize()
                        counts.append(t.rebuild_count() - before)
                        before = t.rebuild_count()
                    ms = 1e3 * (time.perf_counter() - t0) / iters
                    print("%-20s pos rate %-5g rebin_margin %-5.3g rebuilds per 100 iterations: %s   %.3f ms / iteration"
                          % (scene, rate, margin, counts, ms), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "rebuilds":
        rebuilds()
    else:
        adam_timing(int(sys.argv[1]) if len(sys.argv) > 1 else 5)
