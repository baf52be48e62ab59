"""Yardsticks of coarse-to-fine fitting (include/splat2d_coarse.h; csrc/s2d_view_target_math.h).  A helper module, not a test
module:
  * resample(): the NumPy restatement of s2d_view_target_device's area resample, one fp32 operation at a time in the order the
    header states, so that it can be held to the C++ arithmetic and to the kernel on bytes;
  * box_average64(): an independent float64 box average over the same fp32 edges, as two weight matrices and a product;
  * mse255(): main.cpp:796-805 at a view's size, the per-pixel fp32 terms added exactly (math.fsum), as
    loss_ref.sqerr255_exact adds them.
"""
import math

import numpy as np

F = np.float32


def span(origin, zoom, i, size):
    """(lo, hi, first, end) of output pixel i along one axis: [lo, hi) in source coordinates (fp32), source pixels
    first .. end - 1 visited (inside [0, size))."""
    with np.errstate(all="ignore"):
        lo = F(origin) + F(i) / F(zoom)
        hi = F(origin) + F(i + 1) / F(zoom)
    f, e = np.floor(lo), np.ceil(hi)
    f = f if f > 0 else F(0)
    e = e if e < F(size) else F(size)
    f = f if f < F(size) else F(size)
    e = e if e > 0 else F(0)
    return lo, hi, int(f), int(e)


def weight(lo, hi, c):
    """The overlap length of [lo, hi) with source pixel c, one fp32 subtraction."""
    a, b = F(c), F(c + 1)
    l = lo if lo > a else a
    h = hi if hi < b else b
    return F(h - l)


def axis_weights(origin, zoom, out_size, size):
    """Per output pixel of one axis: (first, [fp32 weights of first, first + 1, ...])."""
    out = []
    for i in range(out_size):
        lo, hi, first, end = span(origin, zoom, i, size)
        out.append((first, [weight(lo, hi, c) for c in range(first, end)]))
    return out


def covered(origin, zoom, i):
    """The number of source pixels under output pixel i along one axis, inside the image or not."""
    lo, hi, _, _ = span(origin, zoom, i, 1 << 30)
    return max(int(np.ceil(hi)) - int(np.floor(lo)), 1)


def resample(image, out_width, out_height, origin, zoom):
    """The restatement: (out_height, out_width, 4) float32."""
    image = np.ascontiguousarray(image, dtype=F)
    H, W = image.shape[:2]
    wxs = axis_weights(origin[0], zoom, out_width, W)
    wys = axis_weights(origin[1], zoom, out_height, H)
    zz = F(zoom) * F(zoom)
    out = np.zeros((out_height, out_width, 4), dtype=F)
    for j, (y0, wy) in enumerate(wys):
        for i, (x0, wx) in enumerate(wxs):
            acc = np.zeros(4, dtype=F)
            for dy, vy in enumerate(wy):
                row = np.zeros(4, dtype=F)
                for dx, vx in enumerate(wx):
                    row = row + vx * image[y0 + dy, x0 + dx]
                acc = acc + vy * row
            out[j, i] = acc * zz
    return out


def box_average64(image, out_width, out_height, origin, zoom):
    """The same box average in float64: the overlaps of the fp32 edges with the source pixels as exact differences, two weight
    matrices and one product per channel."""
    image = np.asarray(image, dtype=np.float64)
    H, W = image.shape[:2]

    def matrix(o, out_size, size):
        m = np.zeros((out_size, size), dtype=np.float64)
        c = np.arange(size, dtype=np.float64)
        for i in range(out_size):
            lo, hi, _, _ = span(o, zoom, i, size)
            m[i] = np.clip(np.minimum(float(hi), c + 1.0) - np.maximum(float(lo), c), 0.0, None)
        return m

    mx, my = matrix(origin[0], out_width, W), matrix(origin[1], out_height, H)
    z = float(F(zoom))
    return np.einsum("jy,yxc,ix->jic", my, image, mx) * (z * z)


def block_mean(image, block):
    """The plain fp32 mean of block x block pixels: columns added in ascending order per row, rows in ascending order, times
    1 / block^2 (a power of two)."""
    image = np.ascontiguousarray(image, dtype=F)
    H, W = image.shape[:2]
    oh, ow = -(-H // block), -(-W // block)
    out = np.zeros((oh, ow, 4), dtype=F)
    for j in range(oh):
        for i in range(ow):
            acc = np.zeros(4, dtype=F)
            for y in range(j * block, min((j + 1) * block, H)):
                row = np.zeros(4, dtype=F)
                for x in range(i * block, min((i + 1) * block, W)):
                    row = row + image[y, x]
                acc = acc + row
            out[j, i] = acc * F(1.0 / (block * block))
    return out


def mse255(view, target):
    """sum over pixels of |(view - target).rgb * 255|^2, a float per pixel (main.cpp:801-802), the terms added exactly,
    divided by pixels * 3 (main.cpp:805)."""
    x = np.asarray(view, dtype=F)[..., :3]
    y = np.asarray(target, dtype=F)[..., :3]
    e = ((x - y).astype(F) * F(255.0)).astype(F)
    sq = (e * e).astype(F)
    t = ((sq[..., 0] + sq[..., 1]).astype(F) + sq[..., 2]).astype(F)
    return math.fsum(float(v) for v in t.ravel()) / float(t.size * 3)


def noise_image(W, H, seed):
    return np.random.default_rng(seed).uniform(0.0, 1.0, (H, W, 4)).astype(F)


# ---- the cases of the resample that the CPU and the GPU tests share ---------------------------------------------------------
IMAGES = [(64, 48), (33, 17), (7, 5), (40, 1)]
ZOOMS = [0.5, 0.25, 0.3, 1.0, 2.5, 16.0]
ORIGINS = [(0.0, 0.0), (5.25, 3.5), (-4.0, -4.0)]


BORDER_VIEW = ((-4.0, -4.0), 1.0, 0.0, (72, 56))  # view v4 of view_ref.VIEWS: a border outside the source


def out_size(W, H, zoom):
    """The ceil size of the image at this zoom plus one pixel that overhangs it; at zoom >= 1 no more than 24 x 16 pixels of it
    (the restatement is a Python loop)."""
    ow, oh = math.ceil(W * float(F(zoom))) + 1, math.ceil(H * float(F(zoom))) + 1
    return (min(ow, 24), min(oh, 16)) if zoom >= 1.0 else (ow, oh)


def all_cases():
    """(W, H, seed, origin, zoom, (out_width, out_height)): the cross product, the exact ceil sizes of the odd images at the
    minifying zooms, and the border view v4 of view_ref.VIEWS on the 64 x 48 image."""
    cases = []
    for k, (W, H) in enumerate(IMAGES):
        for zoom in ZOOMS:
            for origin in ORIGINS:
                cases.append((W, H, k, origin, zoom, out_size(W, H, zoom)))
    for k, (W, H) in enumerate(IMAGES):
        for zoom in (0.5, 0.25, 0.3):
            cases.append((W, H, k, (0.0, 0.0), zoom, (math.ceil(W * float(F(zoom))), math.ceil(H * float(F(zoom))))))
    origin, zoom, _, size = BORDER_VIEW
    cases.append((64, 48, 0, origin, zoom, size))
    return cases


CASES = all_cases()
