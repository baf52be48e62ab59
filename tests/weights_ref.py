"""The yardstick of the losses under a pixel-weight plane (include/splat2d_weights.h), in the two
formulations of tests/loss_ref.py with the plane added, sharing nothing but the definition

    L_omega = sum_p omega(p) * sum_c [ w_mse * d^2 / 2 + w_l1 * |d| + w_dssim * (1 - s_c(p)) ]:

  (a) torch_wloss: torch on the CPU, conv2d + autograd; float64 is the reference, float32 what a plain fp32 evaluation loses;
  (b) numpy_wloss: NumPy float64, explicit windowed sums and the hand-derived adjoint, the plane multiplying the three
      derivative maps at the window's centre before the adjoint correlation.

Both return {"grad": (H, W, 3) float64, "mse": the UNWEIGHTED mean of d^2, "wmse", "l1", "dssim": the weighted sums over
3 * H * W (None when not formed; wmse always), "total": L_omega / (3 H W), "weight_sum"}.  Also the planes and the scenes the
CPU and the GPU tests share.
"""
import math

import numpy as np

import loss_ref as LR
import oracle_lib as O

SIZES = {"7x5": (7, 5), "40x1": (40, 1), "33x17": (33, 17), "96x80": (96, 80)}
WEIGHTINGS = [(1.0, 0.0, 0.0), (0.0, 0.8, 0.2), (0.5, 0.3, 0.2)]


def _total(w, wmse, l1, dssim):
    t = 0.0
    if w[0] > 0:
        t += w[0] * 0.5 * wmse
    if w[1] > 0:
        t += w[1] * l1
    if w[2] > 0:
        t += w[2] * dssim
    return t


# ---- (a) torch, conv2d + autograd -------------------------------------------------------------------------------------------
def torch_wloss(x, y, omega, weights, dtype="float64"):
    import torch
    dt = getattr(torch, dtype)
    w_mse, w_l1, w_dssim = (float(v) for v in weights)
    xt = torch.from_numpy(np.ascontiguousarray(np.asarray(x)[..., :3])).to(dt).permute(2, 0, 1)[None].clone().requires_grad_(True)
    yt = torch.from_numpy(np.ascontiguousarray(np.asarray(y)[..., :3])).to(dt).permute(2, 0, 1)[None]
    om = torch.from_numpy(np.ascontiguousarray(omega)).to(dt)[None, None].expand(1, 3, -1, -1)
    n3 = float(xt.numel())
    d = xt - yt
    mse = (d * d).sum() / n3
    wmse = (om * (d * d)).sum() / n3
    l1 = (om * d.abs()).sum() / n3 if w_l1 > 0 else None
    dssim, s = None, None
    if w_dssim > 0:
        k = torch.from_numpy(LR.window2d()).to(dt)[None, None].expand(3, 1, 11, 11).contiguous()

        def conv(a):
            return torch.nn.functional.conv2d(a, k, padding=LR.RADIUS, groups=3)
        mux, muy = conv(xt), conv(yt)
        vx, vy, cxy = conv(xt * xt) - mux * mux, conv(yt * yt) - muy * muy, conv(xt * yt) - mux * muy
        s = ((2 * mux * muy + LR.C1) * (2 * cxy + LR.C2)) / ((mux * mux + muy * muy + LR.C1) * (vx + vy + LR.C2))
        dssim = (om * (1 - s)).sum() / n3
    L = 0
    if w_mse > 0:
        L = L + w_mse * 0.5 * (om * (d * d)).sum()
    if w_l1 > 0:
        L = L + w_l1 * (om * d.abs()).sum()
    if w_dssim > 0:
        L = L + w_dssim * (om * (1 - s)).sum()
    L.backward()
    f = lambda v: None if v is None else float(v.detach())
    out = {"grad": xt.grad[0].permute(1, 2, 0).double().numpy().copy(), "mse": f(mse), "wmse": f(wmse), "l1": f(l1), "dssim": f(dssim),
           "weight_sum": float(np.asarray(omega, dtype=np.float64).sum())}
    out["total"] = _total((w_mse, w_l1, w_dssim), out["wmse"], out["l1"], out["dssim"])
    return out


# ---- (b) NumPy, explicit sums and the adjoint by hand ---------------------------------------------------------------------------
def numpy_wloss(x, y, omega, weights):
    w_mse, w_l1, w_dssim = (float(v) for v in weights)
    x = np.asarray(x)[..., :3].astype(np.float64)
    y = np.asarray(y)[..., :3].astype(np.float64)
    om = np.asarray(omega, dtype=np.float64)[..., None]
    n3 = float(x.size)
    d = x - y
    grad = np.zeros_like(x)
    mse = float((d * d).sum() / n3)
    wmse = float((om * (d * d)).sum() / n3)
    l1 = dssim = None
    if w_mse > 0:
        grad += om * (w_mse * d)
    if w_l1 > 0:
        l1 = float((om * np.abs(d)).sum() / n3)
        grad += om * (w_l1 * np.sign(d))
    if w_dssim > 0:
        mux, muy, exx, eyy, exy = LR.wsum(x), LR.wsum(y), LR.wsum(x * x), LR.wsum(y * y), LR.wsum(x * y)
        a1, a2 = 2 * mux * muy + LR.C1, 2 * (exy - mux * muy) + LR.C2
        b1, b2 = mux * mux + muy * muy + LR.C1, (exx - mux * mux) + (eyy - muy * muy) + LR.C2
        s = a1 * a2 / (b1 * b2)
        dssim = float((om * (1 - s)).sum() / n3)
        # the derivatives of s at a window centre q (tests/loss_ref.py); the loss counts centre q with omega(q), so the plane
        # multiplies the three maps AT THE CENTRE, and x(p) collects them from every centre within its window
        ds_dmu = (2 * muy * a2 - 2 * muy * a1) / (b1 * b2) - s * (2 * mux / b1) + s * (2 * mux / b2)
        ds_dexx = -s / b2
        ds_dexy = 2 * a1 / (b1 * b2)
        grad += w_dssim * -(LR.wsum(om * ds_dmu) + 2 * x * LR.wsum(om * ds_dexx) + y * LR.wsum(om * ds_dexy))
    return {"grad": grad, "mse": mse, "wmse": wmse, "l1": l1, "dssim": dssim, "total": _total((w_mse, w_l1, w_dssim), wmse, l1, dssim),
            "weight_sum": float(om.sum())}


# ---- the weighted sums of the exact products (what a double sum of them, in any order, is within 2 (n - 1) 2^-53 relative of) ----
def weighted_sums_exact(x, y, omega):
    """-> (sum omega, sum omega * sqerr255, sum omega * |d|) with math.fsum over exact products: sqerr255 the fp32 value of
    main.cpp:801-802 per pixel, |d| the exact |x - y| of fp32 values summed over the three channels in double (rounded twice, each
    within 2^-53), omega fp32.  Fractions would be exact to the last bit; the bound of the tests leaves room for these."""
    x = np.asarray(x, dtype=np.float32)[..., :3]
    y = np.asarray(y, dtype=np.float32)[..., :3]
    om = np.asarray(omega, dtype=np.float32).astype(np.float64)
    e = ((x - y).astype(np.float32) * np.float32(255.0)).astype(np.float32)
    sq = (e * e).astype(np.float32)
    t = ((sq[..., 0] + sq[..., 1]).astype(np.float32) + sq[..., 2]).astype(np.float32).astype(np.float64)
    ad = np.abs(x.astype(np.float64) - y.astype(np.float64))
    l1 = (ad[..., 0] + ad[..., 1]) + ad[..., 2]
    return (math.fsum(om.ravel()), math.fsum((om * t).ravel()), math.fsum((om * l1).ravel()))


# ---- planes -------------------------------------------------------------------------------------------------------------------
def random_plane(W, H, seed):
    """Uniform in [0, 2], float32."""
    return np.random.default_rng(1000 + seed).uniform(0.0, 2.0, (H, W)).astype(np.float32)


def binary_mask(W, H):
    """1 where the pixel counts, 0 elsewhere: an edge at x = 32 (the border of two loss tiles) and one inside a tile, at
    x = min(W, 32) // 2 on the lower half of the rows."""
    yy, xx = np.mgrid[0:H, 0:W]
    m = np.ones((H, W), dtype=np.float32)
    m[xx >= 32] = 0.0
    m[(yy >= H // 2) & (xx < min(W, 32) // 2)] = 0.0
    assert m.any() and not m.all()
    return m


def plane(kind, W, H, seed=0):
    if kind == "random":
        return random_plane(W, H, seed)
    if kind == "mask":
        return binary_mask(W, H)
    if kind == "ones":
        return np.ones((H, W), dtype=np.float32)
    raise KeyError(kind)


RANDOM_SCENES = {"7x5": (7, 5, 20, 14), "40x1": (40, 1, 30, 13), "33x17": (33, 17, 200, 11), "96x80": (96, 80, 300, 12)}  # W, H, splats, seed


def noise_scene(size):
    """-> (target (H, W, 4) float32, splats as SPLAT_DTYPE records) of a size of SIZES: the random-splat scene on the noise
    target that tests/test_gpu_pixel_weights.py draws under the same name, number for number."""
    W, H, n, seed = RANDOM_SCENES[size]
    rng = np.random.default_rng(seed)
    s = np.zeros(n, dtype=O.SPLAT_DTYPE)
    s["pos"][:, 0] = rng.uniform(0, W - 1, n)
    s["pos"][:, 1] = rng.uniform(0, H - 1, n)
    s["sx"] = rng.uniform(1.0, 6.0, n)
    s["sy"] = rng.uniform(1.0, 6.0, n)
    s["rot"] = rng.uniform(-np.pi, np.pi, n)
    s["color"] = rng.uniform(0, 1, (n, 3))
    s["opacity"] = rng.uniform(0.1, 1.0, n)
    return np.ascontiguousarray(LR.noise_image(W, H, 100 + seed), dtype=np.float32), s


def image_pair(W, H, content, seed):
    """(x, y) test images of tests/loss_ref.py: uniform noise against noise, or the smooth image against a shifted one."""
    if content == "noise":
        return LR.noise_image(W, H, seed), LR.noise_image(W, H, seed + 50)
    return LR.smooth_image(W, H, 0.3), LR.smooth_image(W, H, 0.0)
