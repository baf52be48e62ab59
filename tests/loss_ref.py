"""The yardstick of the image losses (include/splat2d.h, "image losses"), in two formulations that
share nothing but the definition:

  (a) torch_loss: torch on the CPU, grouped conv2d(padding=5) with the 121-tap window, the gradient by autograd;
      float64 is the reference, float32 on the same inputs is what a plain fp32 evaluation loses (the bar of the GPU tests);
  (b) numpy_loss: NumPy float64, explicit windowed sums over a zero-padded copy and the hand-derived adjoint.

x = image0, y = imageRef as (H, W, >= 3) arrays, .rgb used; L = sum over pixels and channels of
w_mse * d^2 / 2 + w_l1 * |d| + w_dssim * (1 - s); a term whose weight is 0 is neither evaluated nor added.
Both return {"grad": (H, W, 3) float64, "mse", "l1", "dssim": means over 3 * H * W (None when not formed; mse always),
"total", "s": the SSIM map (None without w_dssim)}.
"""
import math

import numpy as np

RADIUS = 5
C1, C2 = 0.01 ** 2, 0.03 ** 2


def window1d():
    g = np.exp(-((np.arange(11, dtype=np.float64) - RADIUS) ** 2) / (2.0 * 1.5 ** 2))
    return g / g.sum()


def window2d():
    g = window1d()
    return np.outer(g, g)


def _total(w, mse, l1, dssim):
    t = 0.0
    if w[0] > 0:
        t += w[0] * 0.5 * mse
    if w[1] > 0:
        t += w[1] * l1
    if w[2] > 0:
        t += w[2] * dssim
    return t


# ---- (a) torch, conv2d + autograd -----------------------------------------------------------------------------------
def torch_loss(x, y, weights, dtype="float64"):
    import torch
    dt = getattr(torch, dtype)
    w_mse, w_l1, w_dssim = (float(v) for v in weights)
    xt = torch.from_numpy(np.ascontiguousarray(np.asarray(x)[..., :3])).to(dt).permute(2, 0, 1)[None].clone().requires_grad_(True)
    yt = torch.from_numpy(np.ascontiguousarray(np.asarray(y)[..., :3])).to(dt).permute(2, 0, 1)[None]
    n3 = float(xt.numel())
    d = xt - yt
    mse = (d * d).sum() / n3
    l1 = d.abs().sum() / n3 if w_l1 > 0 else None
    dssim, s = None, None
    if w_dssim > 0:
        k = torch.from_numpy(window2d()).to(dt)[None, None].expand(3, 1, 11, 11).contiguous()

        def conv(a):
            return torch.nn.functional.conv2d(a, k, padding=RADIUS, groups=3)
        mux, muy = conv(xt), conv(yt)
        vx, vy, cxy = conv(xt * xt) - mux * mux, conv(yt * yt) - muy * muy, conv(xt * yt) - mux * muy
        s = ((2 * mux * muy + C1) * (2 * cxy + C2)) / ((mux * mux + muy * muy + C1) * (vx + vy + C2))
        dssim = (1 - s).sum() / n3
    L = 0
    if w_mse > 0:
        L = L + w_mse * 0.5 * (d * d).sum()
    if w_l1 > 0:
        L = L + w_l1 * d.abs().sum()
    if w_dssim > 0:
        L = L + w_dssim * (1 - s).sum()
    L.backward()
    f = lambda v: None if v is None else float(v.detach())
    out = {"grad": xt.grad[0].permute(1, 2, 0).double().numpy().copy(), "mse": f(mse), "l1": f(l1), "dssim": f(dssim),
           "s": None if s is None else s.detach()[0].permute(1, 2, 0).double().numpy().copy()}
    out["total"] = _total((w_mse, w_l1, w_dssim), out["mse"], out["l1"], out["dssim"])
    return out


# ---- (b) NumPy, explicit sums and the adjoint by hand ---------------------------------------------------------------
def wsum(a):
    """(w * a)(p) = sum_{i,j} w[i,j] a(p + (i-5, j-5)), a = 0 outside the image; per channel."""
    H, W = a.shape[:2]
    pad = np.zeros((H + 2 * RADIUS, W + 2 * RADIUS) + a.shape[2:], dtype=np.float64)
    pad[RADIUS:RADIUS + H, RADIUS:RADIUS + W] = a
    w = window2d()
    out = np.zeros_like(a, dtype=np.float64)
    for i in range(11):
        for j in range(11):
            out += w[i, j] * pad[i:i + H, j:j + W]
    return out


def numpy_loss(x, y, weights):
    w_mse, w_l1, w_dssim = (float(v) for v in weights)
    x = np.asarray(x)[..., :3].astype(np.float64)
    y = np.asarray(y)[..., :3].astype(np.float64)
    n3 = float(x.size)
    d = x - y
    grad = np.zeros_like(x)
    mse = float((d * d).sum() / n3)
    l1 = dssim = s = None
    if w_mse > 0:
        grad += w_mse * d
    if w_l1 > 0:
        l1 = float(np.abs(d).sum() / n3)
        grad += w_l1 * np.sign(d)
    if w_dssim > 0:
        mux, muy, exx, eyy, exy = wsum(x), wsum(y), wsum(x * x), wsum(y * y), wsum(x * y)
        a1, a2 = 2 * mux * muy + C1, 2 * (exy - mux * muy) + C2
        b1, b2 = mux * mux + muy * muy + C1, (exx - mux * mux) + (eyy - muy * muy) + C2
        s = a1 * a2 / (b1 * b2)
        dssim = float((1 - s).sum() / n3)
        # ds at a window centre q, with y fixed, through the three sums that depend on x:
        #   mu_x (a1, a2, b1, b2 all move), w*x^2 (b2 only), w*xy (a2 only)
        ds_dmu = (2 * muy * a2 - 2 * muy * a1) / (b1 * b2) - s * (2 * mux / b1) + s * (2 * mux / b2)
        ds_dexx = -s / b2
        ds_dexy = 2 * a1 / (b1 * b2)
        # x(p) enters the sums of every centre q within the window of p with weight w(p - q); w is symmetric, so the
        # adjoint of the correlation is the correlation; d(x^2) = 2x dx, d(xy) = y dx
        grad += w_dssim * -(wsum(ds_dmu) + 2 * x * wsum(ds_dexx) + y * wsum(ds_dexy))
    return {"grad": grad, "mse": mse, "l1": l1, "dssim": dssim, "s": s, "total": _total((w_mse, w_l1, w_dssim), mse, l1, dssim)}


# ---- the squared error as the reference's own loop forms it ---------------------------------------------------------
def sqerr255_exact(x, y):
    """main.cpp:796-805: lengthSquared((image0 - imageRef) * 255) per pixel in fp32, the fp32 terms added EXACTLY (math.fsum):
    what any double sum of those terms, in any order, is within 2 (n - 1) 2^-53 relative of."""
    x = np.asarray(x, dtype=np.float32)[..., :3]
    y = np.asarray(y, dtype=np.float32)[..., :3]
    e = ((x - y).astype(np.float32) * np.float32(255.0)).astype(np.float32)
    sq = (e * e).astype(np.float32)
    t = ((sq[..., 0] + sq[..., 1]).astype(np.float32) + sq[..., 2]).astype(np.float32)
    return math.fsum(float(v) for v in t.ravel())


# ---- test images ------------------------------------------------------------------------------------------------------
def smooth_image(W, H, phase=0.0):
    """Low-frequency content in [0, 1]: (H, W, 4) float32, .w = 1."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.ones((H, W, 4), dtype=np.float32)
    img[..., 0] = 0.5 + 0.4 * np.sin(0.21 * xx + 0.13 * yy + phase)
    img[..., 1] = 0.5 + 0.4 * np.cos(0.11 * xx - 0.17 * yy + 2.0 * phase)
    img[..., 2] = (xx + 2.0 * yy + 3.0 * phase) / (W + 2.0 * H + 3.0)
    return img


def noise_image(W, H, seed):
    img = np.ones((H, W, 4), dtype=np.float32)
    img[..., :3] = np.random.default_rng(seed).uniform(0.0, 1.0, (H, W, 3))
    return img
