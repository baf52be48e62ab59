#!/usr/bin/env python3
"""CPU tool: per-group learning rates on the ORACLE, to take the bar of tests/test_gpu_optim.py::test_group_rates_lower_the_
final_error -- and the table of DESIGN.md section 15 -- from something other than the code under test.

The squirrel mini (268 x 213), 1024 splats, 300 iterations from init(), opacity off.  Every iteration is the oracle's forward
and backward pass followed by the composite step of tests/optim_ref.py: one s2do_adam_step per distinct rate on copies of
the state, the columns of each parameter group taken from the call made at its rate.  With five equal rates that is the
plain oracle step, byte for byte.  Prints, per set of constant rates (pos, scale, rot, colour, opacity), the MSE the
reference prints for the last iteration, its ratio to the plain run's and the PSNR; then the bar of the GPU test.
  python tools/optim_oracle_schedule.py [iterations] [all]      (all: the whole sweep of DESIGN.md, not only the test's pair)"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib as O  # noqa: E402
import optim_ref as R  # noqa: E402

ITERS = int(sys.argv[1]) if len(sys.argv) > 1 else 300
SWEEP = len(sys.argv) > 2 and sys.argv[2] == "all"
N = 1024
PLAIN = (0.05, 0.05, 0.05, 0.05, 0.05)
RATES = [PLAIN, R.GAIN_RATES]
if SWEEP:
    RATES = [PLAIN, (0.2, 0.05, 0.05, 0.05, 0.05), (0.5, 0.1, 0.05, 0.05, 0.05), R.GAIN_RATES, (1.0, 0.2, 0.1, 0.05, 0.05)]


def run(rates):
    tgt = O.target_rgba32f(O.load_s2di(os.path.join(O.GOLDEN, "squirrel_cls_mini_268x213.s2di")))
    r32 = np.array(rates, dtype=np.float32)
    _, trace = R.oracle_loop(tgt, N, ITERS, lambda t: r32)
    return trace[-1]


if __name__ == "__main__":
    final = {}
    for rates in RATES:
        final[rates] = run(rates)
        ratio = final[rates] / final[PLAIN]
        print("rates %-28s final mse %.4f  ratio %.4f  psnr %.2f dB" % (",".join("%g" % r for r in rates), final[rates], ratio,
                                                                         10.0 * math.log10(255.0 ** 2 / final[rates])), flush=True)
    ratio = final[R.GAIN_RATES] / final[PLAIN]
    print("ratio %.4f  (bar of the GPU test: 1 - half the relative gain = %.4f)" % (ratio, 1.0 - 0.5 * (1.0 - ratio)))
