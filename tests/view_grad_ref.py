"""NumPy restatement of the backward pass through a view (include/splat2d.h "view gradients"; csrc/s2d_view_math.h
view_row_adjoint): the adjoint of the record transform, in the header's operation order and in whatever
float type it is given (float32: the kernel's bits; float64: what the finite-difference test differentiates), and the adjoint of
the supersampling resolve.  Scenes and views are those of tests/view_ref.py."""
import numpy as np

F = np.float32


def rows9(a):
    """A structured splat array as (n, 9) floats (a view, not a copy)."""
    return np.ascontiguousarray(a).view(np.float32).reshape(-1, 9)


def view_rows9(s9, origin, zoom, filter_var=0.0, samples=1, dtype=np.float64):
    """view_ref.view_rows on an (n, 9) array in `dtype`, same operation order."""
    T = dtype
    s = 1 if samples == 0 else int(samples)
    zr = T(T(zoom) * T(s))
    fr = T(T(filter_var) * T(s * s))
    p = np.asarray(s9, dtype=T)
    out = p.copy()
    out[:, 0] = (p[:, 0] - T(origin[0])) * zr
    out[:, 1] = (p[:, 1] - T(origin[1])) * zr
    ax, ay = p[:, 2] * zr, p[:, 3] * zr
    if fr == 0:
        out[:, 2], out[:, 3] = ax, ay
    else:
        sx, sy = np.sqrt(ax * ax + fr), np.sqrt(ay * ay + fr)
        out[:, 2], out[:, 3] = sx, sy
        out[:, 8] = p[:, 8] * ((ax * ay) / (sx * sy))
    return out


def adjoint(s9, g9, origin, zoom, filter_var=0.0, samples=1, dtype=np.float32, alive=None):
    """view_row_adjoint for every row: the gradient g9 (n, 9) with respect to the view's records as the gradient with respect
    to the source records s9 (n, 9).  One operation at a time, in the header's order.  alive: rows with False are left +0 (the
    kernel skips them)."""
    T = dtype
    s = 1 if samples == 0 else int(samples)
    zr = T(T(zoom) * T(s))
    fr = T(T(filter_var) * T(s * s))
    p, g = np.asarray(s9, dtype=T), np.asarray(g9, dtype=T)
    out = np.zeros_like(g)
    with np.errstate(all="ignore"):
        out[:, 0] = g[:, 0] * zr
        out[:, 1] = g[:, 1] * zr
        out[:, 4:8] = g[:, 4:8]
        if fr == 0:
            out[:, 2] = g[:, 2] * zr
            out[:, 3] = g[:, 3] * zr
            out[:, 8] = g[:, 8]
        else:
            ax, ay = p[:, 2] * zr, p[:, 3] * zr
            sx, sy = np.sqrt(ax * ax + fr), np.sqrt(ay * ay + fr)
            k = (ax * ay) / (sx * sy)
            t = (g[:, 8] * p[:, 8]) * k
            out[:, 2] = zr * (g[:, 2] * (ax / sx) + t * (fr / (ax * (sx * sx))))
            out[:, 3] = zr * (g[:, 3] * (ay / sy) + t * (fr / (ay * (sy * sy))))
            out[:, 8] = g[:, 8] * k
    if alive is not None:
        out[~np.asarray(alive, dtype=bool)] = 0
    return out


def expand(u, samples):
    """The adjoint of view_ref.resolve: the gradient of an output pixel to every sample of its block, times 0.25f once per
    resolve level (exact multiplications); (h, w, 4) -> (h * samples, w * samples, 4) in u's dtype."""
    u = np.asarray(u)
    if samples == 1:
        return u.copy()
    out = np.repeat(np.repeat(u, samples, axis=0), samples, axis=1)
    for _ in range({2: 1, 4: 2}[samples]):
        out = out * u.dtype.type(0.25)
    return np.ascontiguousarray(out)


def resolve64(img, samples):
    """view_ref.resolve in float64 on the three colour channels (for the adjoint identity)."""
    img = np.asarray(img, dtype=np.float64)
    for _ in range({1: 0, 2: 1, 4: 2}[samples]):
        img = ((img[0::2, 0::2] + img[0::2, 1::2]) + (img[1::2, 0::2] + img[1::2, 1::2])) * 0.25
    return img


def signed_upstream(h, w, seed=0):
    """A signed dL/d(view) with a third of its columns zero (like the masked Charbonnier upstream of
    tests/test_gpu_image_grads.py), RGBA32F, .w = 0."""
    rng = np.random.default_rng(1000 + seed)
    u = np.zeros((h, w, 4), dtype=F)
    u[..., :3] = rng.uniform(-1.0, 1.0, (h, w, 3)).astype(F)
    u[:, 3 * np.arange(w) < w] = 0
    return u


def random_record_grads(n, seed=0):
    """(n, 9) float32 gradients with zeros (whole rows and single scalars) and negative values."""
    rng = np.random.default_rng(2000 + seed)
    g = (rng.standard_normal((n, 9)) * rng.choice([1e-4, 1.0, 300.0], (n, 1))).astype(F)
    g[rng.uniform(size=(n, 9)) < 0.15] = 0
    g[::7] = 0
    return g



# ---- the finite-difference case of the operator (tests/test_gpu_view_grad.py; pinned on the oracle alone in tests/test_view_grad_cpu.py)
FD_VIEW = dict(origin=(0.0, 0.0), zoom=0.5, filter_var=0.75, samples=2)   # view 3's transform x 2 on fd_check's 72 x 56 scene


def box_half(ref):
    """The 2 x 2 box average of an RGBA32F image (even sizes), in double, rounded once."""
    r = np.asarray(ref, dtype=np.float64)
    return (((r[0::2, 0::2] + r[0::2, 1::2]) + (r[1::2, 0::2] + r[1::2, 1::2])) * 0.25).astype(F)


def fd_weights(view_img, half_target, charbonnier_grad, charbonnier_weights):
    """The weights w (h, w, 3) of the loss sum w * view: the gradient, at the tested point, of the weighted Charbonnier loss of
    the view against the half-size target (tests/test_image_grads_cpu.py: the loss the finite-difference method was pinned
    with), held fixed -- so sum w * view is that loss to first order there: masked on a third of the columns, signed, and of
    full size wherever the view is off the target."""
    h, w = view_img.shape[:2]
    return charbonnier_grad(view_img, half_target, charbonnier_weights(h, w))[..., :3].astype(F)
