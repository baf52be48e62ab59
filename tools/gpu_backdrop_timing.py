#!/usr/bin/env python3
"""GPU-box tool: what a backdrop costs, at 4096^2 / 1 M splats, fp32, synthetic target, after 100 iterations
of a plain context whose splats both contexts then hold.  Every figure is the time between two HIP events on the context's stream
(torch's events on a stream of torch's that the context is given); the plain and the backdrop context take turns, repetition by
repetition, each printed, median and min - max at the end of the line.
  (a) s2d_forward with current lists: raster_forward_kernel against backdrop_forward_kernel (constant, then plane);
  (b) one iteration: the plain context's separate launches (s2d_forward, s2d_backward, s2d_adam_step) and its s2d_step (the fused
      launch) against s2d_step of the backdrop context, four iterations per repetition, per iteration;
  (c) s2d_backdrop_grads: the plane's gradient and the three sums, and the sums alone.
The last line of each pair is the ratio of the medians.
  python tools/gpu_backdrop_timing.py [reps] [size] [splats] [iterations]"""
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
PER = 4  # iterations per timed repetition of (b)


def line(name, v):
    print("%-58s ms: %s   median %.3f  min %.3f  max %.3f" % (name, " ".join("%.3f" % x for x in v), statistics.median(v), min(v), max(v)),
          flush=True)
    return statistics.median(v)


stream = torch.cuda.Stream()
with torch.cuda.stream(stream), S2D.Trainer(W, H, N, stream=stream.cuda_stream) as plain, \
        S2D.BackdropTrainer(W, H, N, stream=stream.cuda_stream) as back:

    def once(call):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        call()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b)

    def series(name, calls, warm=2, per=1):
        """calls: [(label, call)]; they alternate, repetition by repetition.  -> the medians."""
        out = {label: [] for label, _ in calls}
        for k in range(warm + reps):
            for label, call in calls:
                ms = once(call) / per
                if k >= warm:
                    out[label].append(ms)
        med = [line("%s, %s" % (name, label), out[label]) for label, _ in calls]
        for (label, _), m in list(zip(calls, med))[1:]:
            print("    %s / %s (medians): %.4f" % (label, calls[0][0], m / med[0]), flush=True)
        return med

    plain.set_target_synthetic()
    back.set_target_synthetic()
    plain.init()
    plain.step(ITERS, want_mse=False)
    plain.synchronize()
    start = plain.get_splats()
    adam = plain.get_adam()
    back.set_splats(start)
    back.set_adam(*adam)
    back.set_backdrop([1.0, 0.5, 0.25])
    print("%d x %d, %d splats, %d iterations, %d repetitions" % (W, H, N, ITERS, reps), flush=True)
    for t in (plain, back):
        t.forward()  # (lists current from here on)
    stream.synchronize()
    series("(a) s2d_forward, current lists", [("plain", plain.forward), ("constant backdrop", back.forward)])
    noise = torch.rand((H, W, 4), dtype=torch.float32, device="cuda")
    stream.synchronize()
    back.set_backdrop_device(noise.data_ptr())
    back.forward()
    series("(a) s2d_forward, current lists", [("plain", plain.forward), ("plane backdrop", back.forward)])

    up = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    back.get_image_rows_device(up.data_ptr())
    up = up - 0.5
    dplane = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    stream.synchronize()
    series("(c) s2d_backdrop_grads", [("plane gradient and sums", lambda: back.backdrop_grads(up.data_ptr(), dplane.data_ptr())),
                                      ("sums alone", lambda: back.backdrop_grads(up.data_ptr(), 0)),
                                      ("plane gradient alone", lambda: back.backdrop_grads(up.data_ptr(), dplane.data_ptr(), want_rgb=False))])

    back.set_backdrop([1.0, 0.5, 0.25])

    def separate():
        for _ in range(PER):
            plain.forward()
            plain.backward()
            plain.adam_step()

    # every candidate moves its context's splats on: the three run on states PER iterations apart, which at this point of a fit
    # costs the same per iteration (the repetitions printed show it)
    series("(b) one iteration", [("plain, separate launches", separate),
                                 ("plain, s2d_step (fused)", lambda: plain.step(PER, want_mse=False)),
                                 ("backdrop, s2d_step", lambda: back.step(PER, want_mse=False))], per=PER)
    plain.synchronize()
    back.synchronize()
