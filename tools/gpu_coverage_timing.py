#!/usr/bin/env python3
"""GPU-box tool: what the coverage channel costs in the two walks, at 4096^2 / 1 M splats, fp32, synthetic
target, after 100 iterations of a plain context whose splats both contexts then hold.  Every figure is the time between two HIP
events on the context's stream (torch's events on a stream of torch's that the context is given); the plain and the coverage
context take turns, repetition by repetition, each printed, median and min - max at the end of the line.
  (a) s2d_forward with current lists: raster_forward_kernel against coverage_forward_kernel;
  (b) s2d_backward, all nine gradients: raster_backward_kernel against coverage_backward_kernel (+ the squared-error sum);
  (c) s2d_backward_image_grads from a caller's gradient, the UPSTREAM kernels of both.
The last line of each pair is the ratio of the medians.
  python tools/gpu_coverage_timing.py [reps] [size] [splats] [iterations]"""
import importlib
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
S2D = importlib.import_module("2dgaussiansplatting_amd")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
W = H = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
N = int(sys.argv[3]) if len(sys.argv) > 3 else 1_000_000
ITERS = int(sys.argv[4]) if len(sys.argv) > 4 else 100


def line(name, v):
    print("%-52s ms: %s   median %.3f  min %.3f  max %.3f" % (name, " ".join("%.3f" % x for x in v), statistics.median(v), min(v), max(v)),
          flush=True)
    return statistics.median(v)


stream = torch.cuda.Stream()
with torch.cuda.stream(stream), S2D.Trainer(W, H, N, stream=stream.cuda_stream) as plain, \
        S2D.Trainer(W, H, N, stream=stream.cuda_stream, coverage=True) as cover:

    def once(call):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        call()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b)

    def pair(name, call_of, warm=2):
        """call_of(trainer) -> the timed call; the two contexts alternate."""
        out = {"plain": [], "coverage": []}
        for k in range(warm + reps):
            for key, t in (("plain", plain), ("coverage", cover)):
                ms = once(call_of(t))
                if k >= warm:
                    out[key].append(ms)
        p = line(name + ", plain", out["plain"])
        c = line(name + ", coverage", out["coverage"])
        print("    coverage / plain (medians): %.4f" % (c / p), flush=True)

    plain.set_target_synthetic()
    cover.set_target_synthetic()
    plain.init()
    plain.step(ITERS, want_mse=False)
    plain.synchronize()
    cover.set_splats(plain.get_splats())
    print("%d x %d, %d splats, %d iterations, %d repetitions" % (W, H, N, ITERS, reps), flush=True)
    for t in (plain, cover):
        t.forward()  # (lists current from here on)
    up = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    plain.get_image_rows_device(up.data_ptr())
    up = up - 0.5  # a gradient image with all four channels at work
    stream.synchronize()
    pair("(a) s2d_forward, current lists", lambda t: t.forward)
    pair("(b) s2d_backward, nine gradients", lambda t: (lambda: t.backward(skip_opacity_grad=False)))
    pair("(c) s2d_backward_image_grads, nine gradients", lambda t: (lambda: t.backward_image_grads(up.data_ptr(), skip_opacity_grad=False)))
    a, b = torch.empty((H, W, 4), dtype=torch.float32, device="cuda"), torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    plain.get_image_rows_device(a.data_ptr())
    cover.get_image_rows_device(b.data_ptr())
    stream.synchronize()
    print("    rgb of the two frames equal in bytes: %s" % bool(torch.equal(a[..., :3].contiguous().view(torch.int32), b[..., :3].contiguous().view(torch.int32))),
          flush=True)
    plain.synchronize()
    cover.synchronize()
