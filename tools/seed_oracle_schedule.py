#!/usr/bin/env python3
"""CPU tool: the reseeding schedule of tests/test_gpu_seed.py::test_reseeding_lowers_the_final_error on the ORACLE, to take
the test's bar from something other than the code under test.

The squirrel mini (268 x 213), 1024 splats, 300 iterations.  Plain: 300 oracle steps.  Reseeded: before iterations 50, 100,
..., 250 the preceding iteration also gathers the density statistics (sum of T * alpha per splat, from the oracle's backward
pass under the upstream gradient (1, 0, 0), as tests/test_gpu_density.py takes them); then the frame of the current
parameters is formed and the starved rows -- weight < 5, the lowest first, at most 102 -- are drawn from the squared error
map (floor 0) at scale 3 with seed k = iteration / 50 and written by the NumPy restatement tests/seed_ref.py.
Prints the two final MSEs (the value the reference prints for iteration 299) and their ratio.
  python tools/seed_oracle_schedule.py [iterations] [threads]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib as O  # noqa: E402
import seed_ref as R  # noqa: E402
import test_image_grads_cpu as IG  # noqa: E402

ITERS = int(sys.argv[1]) if len(sys.argv) > 1 else 300
THREADS = int(sys.argv[2]) if len(sys.argv) > 2 else 1
EVERY, MAX_MOVES, MIN_WEIGHT, SCALE, N = 50, 102, 5.0, 3.0, 1024


def weights(o):
    """sum T * alpha per splat of the current parameters (one statistics pass)."""
    o.forward()
    g = np.zeros_like(o.image0)
    g[..., 0] = 1.0
    keep = o.ref
    o.ref = np.ascontiguousarray(IG.pseudo_target(o.image0, g))
    try:
        return o.backward_stats()[1][:, 5].astype(np.float32)
    finally:
        o.ref = keep


def run(reseed):
    tgt = O.target_rgba32f(O.load_s2di(os.path.join(O.GOLDEN, "squirrel_cls_mini_268x213.s2di")))
    o = O.OracleTrainer(tgt, N)
    mse = None
    for it in range(ITERS):
        stats = None
        if reseed and (it + 1) % EVERY == 0 and it + 1 < ITERS:
            stats = np.zeros((N, 3), dtype=np.float32)
            stats[:, 2] = weights(o)            # the statistics of the iteration about to run
        st, mse = o.step(THREADS)
        assert st == 0
        if stats is not None:
            ids = R.starved(stats, 1, MAX_MOVES, MIN_WEIGHT)
            img = o.forward().copy()
            q, total = R.importance(R.ERROR, tgt, image0=img, squared=True, floor=0)
            rows = R.rows(ids, (it + 1) // EVERY, q, total, tgt, N, SCALE, 0.0)
            if rows is not None and len(ids):
                o.splats.view(np.float32).reshape(-1, 9)[ids] = rows
                o.adams.view(np.float32).reshape(-1, 18)[ids] = 0.0
            print("  before iteration %d: %d rows reseeded (mse %.3f)" % (it + 1, len(ids) if rows is not None else 0, mse), flush=True)
    return mse


plain = run(False)
print("plain    final mse %.4f" % plain, flush=True)
reseeded = run(True)
print("reseeded final mse %.4f" % reseeded)
print("ratio %.4f  (bar of the GPU test: 1 - half the relative gain = %.4f)" % (reseeded / plain, 1.0 - 0.5 * (1.0 - reseeded / plain)))
