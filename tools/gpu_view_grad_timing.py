#!/usr/bin/env python3
"""GPU-box tool: what the backward pass through a view costs beside the fused launch it is modelled on,
at 4096^2 / 1 M splats, fp32, synthetic target, after 200 iterations.  The method of tools/gpu_view_timing.py: every figure is
the time between two HIP events on the context's stream, each repetition printed behind one untimed, min - max at the end.
  (a) s2d_forward_backward with current lists (raster_fused_kernel; S2D_FB_SKIP_IMAGE): the yardstick;
  (c) whole calls of s2d_view_backward_device -- records, projection, list build (one host wait inside), view_gradient_kernel
      and the adjoint of the record transform.
view_gradient_kernel alone (b) has no entry point of its own: run this tool under a kernel trace (rocprofv3 --kernel-trace
--stats -- python tools/gpu_view_grad_timing.py) and read its row beside raster_fused_kernel's.
  python tools/gpu_view_grad_timing.py [reps] [size] [splats] [iterations]"""
import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
S2D = importlib.import_module("2dgaussiansplatting_amd")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
W = H = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
N = int(sys.argv[3]) if len(sys.argv) > 3 else 1_000_000
ITERS = int(sys.argv[4]) if len(sys.argv) > 4 else 200


def line(name, v):
    print("%-58s ms: %s   min %.3f  max %.3f" % (name, " ".join("%.3f" % x for x in v), min(v), max(v)), flush=True)


stream = torch.cuda.Stream()
with torch.cuda.stream(stream), S2D.Trainer(W, H, N, stream=stream.cuda_stream) as t:

    def timed(call, warm=1):
        out = []
        for k in range(warm + reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            call()
            b.record(stream)
            b.synchronize()
            if k >= warm:
                out.append(a.elapsed_time(b))
        return out

    t.set_target_synthetic()
    t.init()
    t.step(ITERS, want_mse=False)
    t.synchronize()
    print("%d x %d, %d splats, %d iterations, %d repetitions" % (W, H, N, ITERS, reps), flush=True)
    t.forward()  # (lists current from here on)
    fused = lambda: t.forward_backward(skip_opacity_grad=False, skip_image=True)
    line("(a) s2d_forward_backward, current lists", timed(fused))

    def whole(name, out_w, out_h, **kw):
        up = torch.rand((out_h, out_w, 4), dtype=torch.float32, device="cuda") - 0.5
        line("(c) " + name, timed(lambda: t.view_backward_device(up.data_ptr(), out_w, out_h, skip_opacity_grad=False, **kw)))

    q = W // 4
    whole("identity view", W, H)
    whole("0.25x at %d^2" % q, q, q, zoom=0.25)
    whole("0.25x at %d^2, samples = 4" % q, q, q, zoom=0.25, samples=4)
    whole("4x crop of the centre into %d^2" % W, W, H, origin=(W * 3 / 8, H * 3 / 8), zoom=4.0)
    line("(a) s2d_forward_backward, current lists (again)", timed(fused))
    t.synchronize()
