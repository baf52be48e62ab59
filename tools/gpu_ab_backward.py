#!/usr/bin/env python3
"""GPU-box tool: the separate backward pass of two library builds on ONE box in ONE call, alternating -- s2d_backward of
build A (the parent) against s2d_backward and s2d_backward_image_grads of build B, each as `iters` calls behind one
s2d_forward of the same frame (4096^2 / 1 M after 30 iterations).  The upstream gradient is image0 - imageRef formed in
torch, so both passes do the same arithmetic; every repetition is printed, so the spread of repeated runs of A is on the
page next to the difference.
  python tools/gpu_ab_backward.py build/libsplat2d_hip_parent.so 2dgaussiansplatting_amd/lib/libsplat2d_hip.so [reps] [iters]"""
import importlib, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
S2D = importlib.import_module("2dgaussiansplatting_amd")
import torch  # noqa: E402  (after the package: one HIP runtime per process)
libs = [os.path.abspath(p) for p in sys.argv[1:3]]
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
iters = int(sys.argv[4]) if len(sys.argv) > 4 else 100
W = H = 4096
N = 1_000_000


def run(path, upstream):
    S2D.use_library(path)
    with S2D.Trainer(W, H, N) as t:
        t.set_target_synthetic(); t.init()
        t.step(30, want_mse=False)
        t.forward()
        if upstream:
            img = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
            x = torch.arange(W, dtype=torch.float32, device="cuda") / W
            y = torch.arange(H, dtype=torch.float32, device="cuda") / H
            ref = torch.stack([x[None, :].expand(H, W), 1.0 - x[None, :].expand(H, W), y[:, None].expand(H, W),
                               torch.ones((H, W), device="cuda")], dim=-1).contiguous()
            torch.cuda.synchronize()
            t.get_image_rows_device(img.data_ptr())
            t.synchronize()
            up = img - ref
            torch.cuda.synchronize()
            call = lambda: t.backward_image_grads(up.data_ptr(), skip_opacity_grad=False)  # noqa: E731
        else:
            call = lambda: t.backward(skip_opacity_grad=False)  # noqa: E731
        for _ in range(5):
            call()
        t.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            call()
        t.synchronize()
        dt = time.perf_counter() - t0
    S2D.use_library()
    return 1e3 * dt / iters


rows = [("A s2d_backward", libs[0], False), ("B s2d_backward", libs[1], False), ("B s2d_backward_image_grads", libs[1], True)]
ms = {name: [] for name, _, _ in rows}
for r in range(reps):
    for name, path, upstream in rows:
        ms[name].append(run(path, upstream))
for name, _, _ in rows:
    v = ms[name]
    print("%-28s ms per call: %s   min %.4f  max %.4f  spread %.2f %%" % (name, " ".join("%.4f" % x for x in v), min(v), max(v),
                                                                       100.0 * (max(v) / min(v) - 1.0)), flush=True)
a = min(ms[rows[0][0]])
for name, _, _ in rows[1:]:
    print("%-28s best against A's best: %+.2f %%" % (name, 100.0 * (min(ms[name]) / a - 1.0)))
