#!/usr/bin/env python3
"""GPU-box tool: what an iteration of coarse-to-fine fitting costs, at 4096^2 / 1 M splats, fp32, synthetic
target, after 200 iterations.  The method of tools/gpu_view_grad_timing.py: every figure is the time between two HIP events on
the context's stream, each repetition printed behind one untimed, min - max at the end; a repetition is ITER_PER_REP iterations
and the figure is per iteration.
  (i)   s2d_step_view at zoom 0.25 and at zoom 0.5 (the library's own target);
  (ii)  the loop a caller wrote before: s2d_view_backward_device(S2D_VIEW_BWD_FROM_TARGET) + s2d_adam_step on the same view;
  (iii) s2d_step;
  (iv)  s2d_view_target_device at both zooms.
view_fit_kernel beside view_gradient_kernel: run this tool under a kernel trace (rocprofv3 --kernel-trace --stats -- python
tools/gpu_coarse_timing.py) and read the two rows.
  python tools/gpu_coarse_timing.py [reps] [size] [splats] [iterations]"""
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
ITER_PER_REP = 4


def line(name, v):
    print("%-64s ms: %s   min %.3f  max %.3f" % (name, " ".join("%.3f" % x for x in v), min(v), max(v)), flush=True)


stream = torch.cuda.Stream()
with torch.cuda.stream(stream), S2D.CoarseTrainer(W, H, N, stream=stream.cuda_stream) as t:

    def timed(call, per=1, warm=1):
        out = []
        for k in range(warm + reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            call()
            b.record(stream)
            b.synchronize()
            if k >= warm:
                out.append(a.elapsed_time(b) / per)
        return out

    t.set_target_synthetic()
    t.init()
    t.step(ITERS, want_mse=False)
    t.synchronize()
    print("%d x %d, %d splats, %d iterations, %d repetitions of %d iterations" % (W, H, N, ITERS, reps, ITER_PER_REP), flush=True)
    line("(iii) s2d_step", timed(lambda: t.step(ITER_PER_REP, want_mse=False), ITER_PER_REP))
    for zoom in (0.25, 0.5):
        ow, oh = int(W * zoom), int(H * zoom)
        small = torch.empty((oh, ow, 4), dtype=torch.float32, device="cuda")
        line("(iv)  s2d_view_target_device, zoom %g (%d^2)" % (zoom, ow), timed(lambda: t.view_target_device(small.data_ptr(), ow, oh, zoom=zoom)))
        line("(i)   s2d_step_view, zoom %g" % zoom, timed(lambda: t.step_view(ITER_PER_REP, ow, oh, zoom=zoom), ITER_PER_REP))

        def callers_loop():
            for _ in range(ITER_PER_REP):
                t.view_backward_device(small.data_ptr(), ow, oh, zoom=zoom, from_target=True, skip_opacity_grad=True)
                t.adam_step()

        line("(ii)  view_backward_device(from_target) + adam_step, zoom %g" % zoom, timed(callers_loop, ITER_PER_REP))
        line("(i)   s2d_step_view, zoom %g (again)" % zoom, timed(lambda: t.step_view(ITER_PER_REP, ow, oh, zoom=zoom), ITER_PER_REP))
    t.view_release()
    line("(iii) s2d_step (again)", timed(lambda: t.step(ITER_PER_REP, want_mse=False), ITER_PER_REP))
    t.synchronize()
