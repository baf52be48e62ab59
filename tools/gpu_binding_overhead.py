#!/usr/bin/env python3
"""GPU-box tool: what one call through the Python binding costs, where an iteration is short enough for the host to show.

The mini scene (tests/golden/squirrel_cls_mini_268x213.s2di, 268 x 213, 2 000 splats, the as-shipped configuration) runs at
some tens of microseconds per iteration, so the ctypes call, the status check and the flag helpers of the binding are a
visible share of it -- which bench.py at 4096^2 hides.  Two loops, each timed as a whole with one synchronize() at the end:

  step:      `--calls` calls of step(1, want_mse=False)
  separate:  `--calls` rounds of forward_backward() + adam_step()

and the result is one JSON line with the microseconds per call (per round for the second loop).  To compare two versions of
the binding, run the tool from each tree against the SAME library file (S2D_LIBRARY=<path>), alternating, several times
each: the differences between repeated runs of one version are the yardstick for the difference between the two.

  python tools/gpu_binding_overhead.py [--calls 3000] [--warmup 300]
"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
S2D = importlib.import_module("2dgaussiansplatting_amd")
import oracle_lib as O  # noqa: E402  (fixture loading only)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=3000)
    ap.add_argument("--warmup", type=int, default=300)
    args = ap.parse_args()
    tgt = O.target_rgba32f(O.load_s2di(os.path.join(O.GOLDEN, "squirrel_cls_mini_268x213.s2di")))
    H, W = tgt.shape[:2]
    out = {"scene": "%dx%d" % (W, H), "splats": 2000, "calls": args.calls, "package": os.path.relpath(os.path.dirname(S2D.__file__), ROOT),
           "library": os.path.relpath(os.environ.get("S2D_LIBRARY") or S2D._build.LIB_PATH, ROOT)}  # (relative to this tree)
    with S2D.Trainer(W, H, 2000) as t:
        t.set_target(tgt)
        t.init()
        for _ in range(args.warmup):
            t.step(1, want_mse=False)
        t.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            t.step(1, want_mse=False)
        t.synchronize()
        out["step_us_per_call"] = round(1e6 * (time.perf_counter() - t0) / args.calls, 3)
        for _ in range(args.warmup):
            t.forward_backward()
            t.adam_step()
        t.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            t.forward_backward()
            t.adam_step()
        t.synchronize()
        out["separate_us_per_round"] = round(1e6 * (time.perf_counter() - t0) / args.calls, 3)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
