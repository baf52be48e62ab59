#!/usr/bin/env python3
"""GPU-box tool: sha256 of what deterministic training leaves (MSE trace, splats, Adam moments, framebuffer, tile lists) on
a few workloads that rebuild the lists often, for the library S2D_LIBRARY names (default: the tree's).  Two libraries that
compute the same print the same lines.

  S2D_LIBRARY=build/libsplat2d_hip_parent.so python tools/gpu_det_hash.py; python tools/gpu_det_hash.py
"""
import hashlib
import importlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
S2D = importlib.import_module("2dgaussiansplatting_amd")
for W, H, n, iters, kw in [(2048, 2048, 250_000, 60, {}), (2048, 2048, 250_000, 20, {"rebin_interval": 1}),
                           (535, 426, 50_000, 200, {"generic_binning": True}), (268, 213, 1024, 300, {}),
                           (268, 213, 2000, 30, {"chunk_pairs": 3000})]:
    with S2D.Trainer(W, H, n, deterministic=True, **kw) as t:
        t.set_target_synthetic()
        t.init()
        tr = t.step(iters)
        h = hashlib.sha256()
        for a in (tr, t.get_splats(), t.get_adam()[0], t.get_image()):
            h.update(a.tobytes())
        st = t.stats()
        if "chunk_pairs" not in kw:
            t.forward()
            for a in t.tile_lists()[2:]:
                h.update(a.tobytes())
        print(W, H, n, iters, kw, h.hexdigest()[:20], "pairs", st["pairs_binned"], "cap", st["pairs_capacity"], "rebins", st["rebins"], flush=True)
