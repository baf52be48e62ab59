#!/usr/bin/env python3
"""GPU-box tool: what a view costs beside the forward pass it is modelled on, at 4096^2 / 1 M splats,
fp32, synthetic target, after 200 iterations.  Every figure is the time between two HIP events on the context's stream (torch's
events on a stream of torch's that the context is given), each repetition printed, min - max at the end of the line.
  (a) raster_forward_kernel through s2d_forward with current lists: the yardstick;
  (b) the view raster kernel alone on the identity view (s2d_debug_view_raster, include/splat2d_test.h);
  (c) whole calls of s2d_render_view_device -- records, projection, list build (one host wait inside) and raster.
  python tools/gpu_view_timing.py [reps] [size] [splats] [iterations]"""
import ctypes as C
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
    line("(a) s2d_forward, current lists", timed(t.forward))

    buf = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    ident = t._view_config(W, H)
    t.render_view_device(buf.data_ptr(), W, H)
    line("(b) view raster kernel alone, identity view", timed(lambda: t._ck(t.L.s2d_debug_view_raster(t._h, C.byref(ident), C.c_void_p(buf.data_ptr())))))
    t.forward()
    img = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    t.get_image_rows_device(img.data_ptr())
    stream.synchronize()
    print("    identity view == image0 in bytes: %s" % bool(torch.equal(buf.view(torch.int32), img.view(torch.int32))), flush=True)

    def whole(name, out_w, out_h, **kw):
        rgba8 = kw.get("rgba8", False)
        out = torch.empty((out_h, out_w, 4), dtype=torch.uint8 if rgba8 else torch.float32, device="cuda")
        line("(c) " + name, timed(lambda: t.render_view_device(out.data_ptr(), out_w, out_h, **kw)))

    q = W // 4
    whole("identity view", W, H)
    whole("4x zoom of the centre into %d^2" % W, W, H, origin=(W * 3 / 8, H * 3 / 8), zoom=4.0)
    whole("4x zoom of the centre into %d^2, RGBA8" % W, W, H, origin=(W * 3 / 8, H * 3 / 8), zoom=4.0, rgba8=True)
    whole("0.25x thumbnail at %d^2" % q, q, q, zoom=0.25)
    whole("0.25x thumbnail at %d^2, samples = 4" % q, q, q, zoom=0.25, samples=4)
    whole("0.25x thumbnail at %d^2, samples = 4, RGBA8" % q, q, q, zoom=0.25, samples=4, rgba8=True)
    line("(a) s2d_forward, current lists (again)", timed(t.forward))
    t.step(2, want_mse=False)  # (the context trains on)
    t.synchronize()
