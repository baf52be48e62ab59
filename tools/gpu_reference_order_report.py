"""Default mode against the reference-order validation mode (S2D_CFG_REFERENCE_ORDER), measured on a GPU, not asserted.

    python tools/gpu_reference_order_report.py [--out profiles/r07/r07_parity_report.txt] [--iters 300]

The mode's gradients, state and trace are the reference's bytes (tests/test_gpu_reference_order.py), so it is the
yardstick here.  Per scene (mini / 1024, mini / 2000, 535x426 / 50 k):
  * from the mode's own state at iterations 0 and 20, one forward + backward in either mode: maximum and 99.9th
    percentile ulp distance of the default mode's gradients, per component;
  * both modes run from init(): the first iteration at which the "%.4f" trace (main.cpp:807) differs;
  * what an iteration costs in either mode, and the ordered squared-error chain alone at 4096 x 4096.
Needs the built library and an MI355X; the oracle is not used.
"""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib as O  # noqa: E402  (fixture loading only)

S2D = importlib.import_module("2dgaussiansplatting_amd")
COMPONENTS = ["pos.x", "pos.y", "sx", "sy", "rot", "color.r", "color.g", "color.b", "opacity"]


def ordered(a):
    """binary32 -> integers whose difference is the distance in units in the last place (+0 and -0 coincide)."""
    i = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def ulp_distance(a, b):
    return np.abs(ordered(a) - ordered(b))


def grads_of(W, H, n, tgt, splats, adam, **kw):
    with S2D.Trainer(W, H, n, **kw) as t:
        t.set_target(tgt)
        t.set_splats(splats)
        t.set_adam(*adam)
        t.forward()
        t.backward(skip_opacity_grad=False)
        return t.get_grads().view(np.float32).reshape(-1, 9).copy()


def scene_report(name, tgt, n, iters, out):
    H, W = tgt.shape[:2]
    out.append("== %s: %dx%d, %d splats" % (name, W, H, n))
    with S2D.Trainer(W, H, n, reference_order=True) as ref:
        ref.set_target(tgt)
        ref.init()
        for it in (0, 20):
            if it:
                ref.step(it, want_mse=False)
            splats, adam = ref.get_splats(), ref.get_adam()
            assert adam[3] == it
            want = grads_of(W, H, n, tgt, splats, adam, reference_order=True)
            got = grads_of(W, H, n, tgt, splats, adam)
            d = ulp_distance(got, want)
            out.append("  iteration %d: ulp distance of the default mode's gradients from the mode's (max / 99.9th percentile / share equal)" % it)
            for k, c in enumerate(COMPONENTS):
                out.append("    %-8s %12d %10.1f %8.4f" % (c, d[:, k].max(), np.percentile(d[:, k], 99.9), float((d[:, k] == 0).mean())))
    traces, rates = {}, {}
    for mode, kw in (("default", {}), ("reference_order", {"reference_order": True})):
        with S2D.Trainer(W, H, n, **kw) as t:
            t.set_target(tgt)
            t.init()
            t.synchronize()
            t0 = time.perf_counter()
            traces[mode] = t.step(iters)  # (ends in a device synchronise: the trace is read back)
            rates[mode] = (time.perf_counter() - t0) / iters
    a, b = ["%.4f" % v for v in traces["default"]], ["%.4f" % v for v in traces["reference_order"]]
    diff = [k for k in range(iters) if a[k] != b[k]]
    out.append("  \"%%.4f\" trace over %d iterations: %s" % (iters, "first difference at iteration %d (%s vs %s), %d lines differ"
                                                            % (diff[0], a[diff[0]], b[diff[0]], len(diff)) if diff else "no line differs"))
    out.append("  last line: default %s, reference order %s" % (a[-1], b[-1]))
    out.append("  ms per iteration, first call of %d iterations, list builds included: default %.3f, reference order %.3f"
               % (iters, 1e3 * rates["default"], 1e3 * rates["reference_order"]))


def sqerr_chain_report(out):
    """4096 x 4096 with 64 splats: the backward pass is the squared error and little else."""
    W = H = 4096
    ms = {}
    for mode, kw in (("default", {}), ("reference_order", {"reference_order": True})):
        with S2D.Trainer(W, H, 64, **kw) as t:
            t.set_target_synthetic()
            t.init()
            t.forward()
            t.backward()
            t.mse()
            t0 = time.perf_counter()
            for _ in range(3):
                t.backward()
            t.mse()
            ms[mode] = 1e3 * (time.perf_counter() - t0) / 3
    out.append("== 4096x4096, 64 splats: ms per backward pass (the ordered squared-error chain of 16.8 M pixels dominates the mode's)")
    out.append("  default %.3f, reference order %.3f" % (ms["default"], ms["reference_order"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07", "r07_parity_report.txt"))
    ap.add_argument("--iters", type=int, default=300)
    a = ap.parse_args()
    mini = O.target_rgba32f(O.load_s2di(os.path.join(O.GOLDEN, "squirrel_cls_mini_268x213.s2di")))
    full = O.target_rgba32f(O.load_s2di(os.path.join(O.GOLDEN, "squirrel_cls_535x426.s2di")))
    out = ["default mode against S2D_CFG_REFERENCE_ORDER (tools/gpu_reference_order_report.py); measured, not asserted"]
    for name, tgt, n in (("mini / 1024", mini, 1024), ("mini / 2000", mini, 2000), ("535x426 / 50 k", full, 50000)):
        scene_report(name, tgt, n, a.iters, out)
        open(a.out, "w").write("\n".join(out) + "\n")  # (what is measured so far survives a later failure)
    sqerr_chain_report(out)
    open(a.out, "w").write("\n".join(out) + "\n")
    print("\n".join(out))


if __name__ == "__main__":
    main()
