#!/usr/bin/env python3
"""GPU-box tool: how much of an Adam launch's traffic belongs to splats the launch cannot change.

A splat is INERT in a launch when its nine gradient words and its eighteen moments are all +0 (what adam_kernel reads off
the gradients and its `dormant` byte).  At the given iterations of the bench workload this reads the gradients a
forward + backward pass left and the moments back to the host (a one-off read-back: the library carries no counter) and
prints the inert share of the splats, of whole 256-splat blocks, and of the 16-byte lines / 64- and 128-byte sectors of
each array that hold words of inert records only -- the lines the launch does not move, and what that can save in HBM.

  python tools/gpu_adam_inert_stats.py [W H n] [--at 10,60,109,210]
"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
S2D = importlib.import_module("2dgaussiansplatting_amd")


def dead_share(inert, record_bytes, unit_bytes):
    """Share of the unit_bytes-sized, aligned pieces of an array of record_bytes-sized records that hold inert records only."""
    n = inert.shape[0]
    units = (n * record_bytes + unit_bytes - 1) // unit_bytes
    live_at = np.nonzero(~inert)[0].astype(np.int64)
    first = live_at * record_bytes // unit_bytes
    last = ((live_at + 1) * record_bytes - 1) // unit_bytes
    touched = np.zeros(units + 1, dtype=np.int32)
    np.add.at(touched, first, 1)
    np.add.at(touched, last + 1, -1)
    return float((np.cumsum(touched[:units]) == 0).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("size", nargs="*", type=int, default=[4096, 4096, 1_000_000])
    ap.add_argument("--at", default="10,60,109,210")
    args = ap.parse_args()
    W, H, n = args.size
    at = sorted(int(x) for x in args.at.split(","))
    print("size %dx%d n=%d" % (W, H, n))
    with S2D.Trainer(W, H, n) as t:
        t.set_target_synthetic()
        t.init()
        done = 0
        for it in at:
            if it > done:
                t.step(it - done, want_mse=False)
                done = it
            t.forward_backward()
            t.synchronize()
            g = t.get_grads().view(np.uint32).reshape(n, 9)
            m = t.get_adam()[0].view(np.uint32).reshape(n, 18)
            zero_g = ~g.any(axis=1)
            inert = zero_g & ~m.any(axis=1)
            blocks = np.add.reduceat(inert.astype(np.int32), np.arange(0, n, 256))
            sizes = np.minimum(256, n - np.arange(0, n, 256))
            print("iteration %d: zero gradient %.1f%%  inert %.1f%% of the splats; %.1f%% of the 256-splat blocks wholly inert, "
                  "%.1f%% of the inert splats in such blocks" % (it, 100 * zero_g.mean(), 100 * inert.mean(), 100 * (blocks == sizes).mean(),
                                                               100.0 * blocks[blocks == sizes].sum() / max(int(inert.sum()), 1)))
            q = np.quantile(np.nonzero(inert)[0], [0.1, 0.5, 0.9]) if inert.any() else [0, 0, 0]
            print("    index of the inert splats, 10 / 50 / 90 %%: %d / %d / %d" % tuple(int(x) for x in q))
            moved = 0.0
            for name, rec, passes in (("params", 36, 2), ("moments", 72, 2), ("proj", 64, 1)):
                d = [dead_share(inert, rec, u) for u in (16, 64, 128)]
                moved += passes * rec * (1 - d[1])
                print("    %-8s lines of inert records only: %.1f%% of 16 B, %.1f%% of 64 B, %.1f%% of 128 B" % ((name,) + tuple(100 * x for x in d)))
            gz = [dead_share(zero_g, 36, u) for u in (16, 64, 128)]
            print("    gradient lines already +0 (no store): %.1f%% of 16 B, %.1f%% of 64 B, %.1f%% of 128 B" % tuple(100 * x for x in gz))
            print("    bytes per splat at 64-B granularity: %.0f of 352 (gradients read in full, stored where not +0)"
                  % (36 + 36 * (1 - gz[1]) + moved))
            t.adam_step()
            done += 1


if __name__ == "__main__":
    main()
