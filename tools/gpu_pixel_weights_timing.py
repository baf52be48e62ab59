"""What a pixel-weight plane costs (measured, not asserted).  On one MI355X, by default 4096 x 4096 with
10^6 splats from init() after a few iterations:

  (a) the loss pass alone (s2d_loss_image_grads_device) for the weightings (1, 0, 0) and (0, 0.8, 0.2): under a plane, without
      one, and -- with --parent-lib -- both again on a build of the parent commit (which must have the plane's symbols: a
      process that fails ends the series), tree and parent alternating, each in a process of its own, one after the other in the same session;
  (b) one iteration: s2d_step under a plane against s2d_step_loss (1, 0, 0) without one (the same separate launches), and the
      plain fused s2d_step beside them.

    python tools/gpu_pixel_weights_timing.py [--size 4096] [--splats 1000000] [--reps 9] [--parent-lib build/libsplat2d_hip_parent.so]
                                             [--out profiles/r29/pixel_weights_timing_1.json]

Wall clock around `calls` queued calls and one wait for the stream, per repetition; medians (min - max) in ms per call.
"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WEIGHTINGS = [(1.0, 0.0, 0.0), (0.0, 0.8, 0.2)]


def _stats(ms):
    return {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}


def measure(role, size, splats, reps, calls):
    """role "plane": this process's library with a plane; "plain": without (the library S2D_LIBRARY names, or the tree's)."""
    import torch
    S2D = importlib.import_module("2dgaussiansplatting_amd")
    weighted = role == "plane"
    t = S2D.Trainer(size, size, splats)
    if weighted:
        S2D.WeightedTrainer.of(t)
    t.set_target_synthetic()
    t.init()
    t.step(10, want_mse=False)
    if weighted:
        t.set_pixel_weights(np.random.default_rng(1).uniform(0.0, 2.0, (size, size)).astype(np.float32))
    buf = torch.empty((size, size, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    out = {}
    t.forward()
    for w in WEIGHTINGS:
        t.loss_image_grads_device(buf.data_ptr(), *w)   # (allocates on first use)
        t.synchronize()
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter()
            for _ in range(calls):
                t.loss_image_grads_device(buf.data_ptr(), *w)
            t.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3 / calls)
        out["loss_pass %s" % (w,)] = _stats(ms)
    steps = {"s2d_step": lambda: t.step(calls, want_mse=False)}
    if not weighted:
        steps["s2d_step_loss (1, 0, 0)"] = lambda: t.step_loss(calls, 1.0, 0.0, 0.0, want=False)
    for name, f in steps.items():
        f()
        t.synchronize()
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter()
            f()
            t.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3 / calls)
        out[name] = _stats(ms)
    t.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--splats", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--calls", type=int, default=8)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--role", default=None, help="internal: measure in this process and print JSON")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.role:
        print("RESULT " + json.dumps(measure(a.role, a.size, a.splats, a.reps, a.calls)))
        return 0
    runs = [("tree, plane", "plane", None), ("tree, no plane", "plain", None)]
    if a.parent_lib:   # tree and parent alternating, role by role
        parent = os.path.abspath(a.parent_lib)
        runs = [runs[0], ("parent, plane", "plane", parent), runs[1], ("parent, no plane", "plain", parent)]
    result = {"command": " ".join(sys.argv), "size": a.size, "splats": a.splats, "reps": a.reps, "calls": a.calls, "ms_per_call": {}}
    for label, role, lib in runs:   # one process after the other: never two on the card at once
        env = dict(os.environ)
        if lib:
            env["S2D_LIBRARY"] = lib
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--role", role, "--size", str(a.size), "--splats", str(a.splats),
                            "--reps", str(a.reps), "--calls", str(a.calls)], env=env, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            print(r.stdout[-2000:], r.stderr[-2000:], file=sys.stderr)
            return r.returncode   # (nothing more is started after a process that failed)
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
        result["ms_per_call"][label] = json.loads(line[len("RESULT "):])
    text = json.dumps(result, indent=1, sort_keys=True)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
