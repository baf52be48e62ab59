#!/usr/bin/env python3
"""GPU-box tool: what the image losses (s2d_loss_*) cost at 4096^2 / 1 M splats, fp32, synthetic target.
  1. the loss kernels alone (s2d_loss_image_grads_device of one frame), timed with HIP events on the stream they run on,
     as ms per pass and as GB/s of their algorithmic bytes: 32 B in + 16 B out per pixel, plus 36 B written and read for the
     maps when w_dssim > 0;
  2. whole iterations after 30 warm-up iterations, alternating in one process (the method of tools/gpu_ab_backward.py):
     forward + backward + adam_step  against  step_loss(1, 0, 0)  and  step_loss(0, 0.8, 0.2).
Every repetition is printed.  The context works on a torch side stream, so that torch's events bracket its launches.
  python tools/gpu_loss_timing.py [reps] [iters]        (S2D_LOSS_TIMING_KERNELS_ONLY=1 in the environment: part 1 alone)"""
import importlib, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
S2D = importlib.import_module("2dgaussiansplatting_amd")
import torch  # noqa: E402  (after the package: one HIP runtime per process)
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 20
W = H = 4096
N = 1_000_000
PIXELS = W * H

# (a null stream handle would make the context create a stream of its own, which torch's events are not recorded on)
side = torch.cuda.Stream()
with torch.cuda.stream(side), S2D.Trainer(W, H, N, stream=side.cuda_stream) as t:
    t.set_target_synthetic(); t.init()
    t.step(30, want_mse=False)
    t.forward()
    buf = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    for name, w, nbytes in (("L1 + D-SSIM (0, 0.8, 0.2): moments + adjoint + finalize", (0.0, 0.8, 0.2), 120 * PIXELS),
                            ("D-SSIM alone (0, 0, 1)", (0.0, 0.0, 1.0), 120 * PIXELS),
                            ("MSE (1, 0, 0): pointwise + finalize", (1.0, 0.0, 0.0), 48 * PIXELS)):
        for _ in range(3):
            t.loss_image_grads_device(buf.data_ptr(), *w)
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                t.loss_image_grads_device(buf.data_ptr(), *w)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / iters)
        print("%-58s ms per pass: %s   best %.4f = %.0f GB/s of %d algorithmic bytes, terms %s" % (
            name, " ".join("%.4f" % v for v in ms), min(ms), nbytes / (min(ms) * 1e-3) / 1e9, nbytes, t.loss_terms()), flush=True)

    if os.environ.get("S2D_LOSS_TIMING_KERNELS_ONLY"):
        sys.exit(0)

    def sequence():
        t.forward(); t.backward(); t.adam_step()
    rows = [("forward + backward + adam_step", lambda: [sequence() for _ in range(iters)]),
            ("step_loss(1, 0, 0)", lambda: t.step_loss(iters, 1.0, 0.0, 0.0, want=False)),
            ("step_loss(0, 0.8, 0.2)", lambda: t.step_loss(iters, 0.0, 0.8, 0.2, want=False))]
    t.lean_backward = True  # (what step_loss does without optimize_opacity: the opacity gradient is skipped)
    out = {name: [] for name, _ in rows}
    for name, f in rows:  # the allocations of the first loss pass stay out of the timings
        f()
    for _ in range(reps):
        for name, f in rows:
            t.synchronize()
            t0 = time.perf_counter()
            f()
            t.synchronize()
            out[name].append(1e3 * (time.perf_counter() - t0) / iters)
    base = min(out[rows[0][0]])
    for name, _ in rows:
        v = out[name]
        print("%-32s ms per iteration: %s   best %.4f (%+.2f %% against the sequence's best)" % (
            name, " ".join("%.4f" % x for x in v), min(v), 100.0 * (min(v) / base - 1.0)), flush=True)
