"""The cases of tests/golden/loss_bytes.json: what a loss pass writes, byte for byte, as digests and hexadecimal doubles.

tools/record_loss_bytes.py evaluates them on a build of the commit BEFORE a change of the loss kernels and writes the fixture;
tests/test_gpu_loss_bytes.py evaluates them on the tree's library and asks for equality.  The build contracts nothing and
no loss kernel has an atomic, so the bytes follow from the order of the operations in the source: a refactor keeps them.

Cases, the smallest at which each path of the kernels can go wrong:
  scenes     the random-splat scenes of tests/weights_ref.py on the noise target: 7x5 (one partial tile, every window clipped
             on all sides), 40x1 (one row, two tiles across), 33x17 (one column past a tile edge), 96x80 (3 x 3 tiles, one
             whose halo lies wholly inside);
  weightings the pointwise kernel alone ((1, 0, 0), (0, 1, 0), (1, 0.5, 0)), the window kernels alone ((0, 0, 1)) and both
             kinds of term together ((0, 0.8, 0.2), (0.5, 0.3, 0.2));
  planes     none (the unweighted kernels), and the random and the mask plane of weights_ref.plane (the weighted ones);
  images     fp32 and fp16.
"""
import hashlib
import importlib
import json
import os

import numpy as np

import oracle_lib as O
import weights_ref as WR

FIXTURE = os.path.join(O.GOLDEN, "loss_bytes.json")
SCENES = ["7x5", "40x1", "33x17", "96x80"]
WEIGHTINGS = [(1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (1.0, 0.5, 0.0), (0.0, 0.0, 1.0), (0.0, 0.8, 0.2), (0.5, 0.3, 0.2)]
PLANES = ["none", "random", "mask"]
IMAGES = {"fp32": {}, "fp16": {"fp16_images": True}}
GROUPS = [(s, i, p) for s in SCENES for i in sorted(IMAGES) for p in PLANES]


def group_key(scene, images, plane):
    return "%s %s %s" % (scene, images, plane)


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _hex(d, keys):
    return [float(d[k]).hex() for k in keys]


def evaluate(scene, images, plane):
    """One context on the library of the process (S2D_LIBRARY, or the tree's): the forward pass once, then a loss pass per
    weighting -> {"image0": digest, "<weighting>": {"grad": digest of the RGBA32F gradient image, "terms": mse, l1, dssim, total
    of s2d_loss_get, "weighted": weight_sum, mse, l1, dssim, total of s2d_weighted_loss_get (under a plane)}}."""
    import torch
    S2D = importlib.import_module("2dgaussiansplatting_amd")
    tgt, splats = WR.noise_scene(scene)
    H, W = tgt.shape[:2]
    out = {}
    with S2D.WeightedTrainer(W, H, len(splats), **IMAGES[images]) as t:
        t.set_target(tgt)
        t.set_splats(splats.view(S2D.SPLAT_DTYPE))
        if plane != "none":
            t.set_pixel_weights(WR.plane(plane, W, H, seed=W))
        t.forward()
        out["image0"] = _sha(t.get_image_rows())
        for w in WEIGHTINGS:
            buf = torch.full((H, W, 4), float("nan"), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            t.loss_image_grads_device(buf.data_ptr(), *w)
            t.synchronize()
            rec = {"grad": _sha(buf.cpu().numpy()), "terms": _hex(t.loss_terms(), ("mse", "l1", "dssim", "total"))}
            if plane != "none":
                rec["weighted"] = _hex(t.weighted_terms(), ("weight_sum", "mse", "l1", "dssim", "total"))
            out[str(w)] = rec
    return out


def write_fixture(cases, path):
    """{group key: evaluate(...)} as JSON, one line per weighting."""
    groups = ['"%s": {\n%s\n}' % (key, ",\n".join(" %s: %s" % (json.dumps(k), json.dumps(v, sort_keys=True)) for k, v in sorted(g.items())))
              for key, g in sorted(cases.items())]
    with open(path, "w") as f:
        f.write('{"cases": {\n%s\n}}\n' % ",\n".join(groups))


def recorded():
    with open(FIXTURE) as f:
        return json.load(f)
