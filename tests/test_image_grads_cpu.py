"""The backward pass from a caller's image gradient (s2d_backward_image_grads), CPU side:
  * the three device-pointer entry points reject null arguments before they touch a device;
  * the METHOD by which tests/test_gpu_image_grads.py checks an arbitrary upstream gradient is pinned on the oracle alone.

The method.  The oracle (like the reference) can only differentiate L = 1/2 sum (image0 - imageRef)^2, whose dL/dC is
image0 - imageRef (main.cpp:616).  An arbitrary upstream gradient g is therefore handed to it as the PSEUDO-TARGET
imageRef' = fp32(image0 - g): its backward pass then starts from fp32(image0 - imageRef'), which is g up to one rounding
of image0's magnitude, and everything behind that line is the reference's arithmetic.  Here the oracle, with the exact
exponential (main.cpp:51), is shown to produce the derivative of a loss that is NOT the squared error -- a weighted
Charbonnier loss with a masked third of the image -- by the two-step finite-difference rule of fd_check.check, restated
below for a general loss (same STEPS, same thresholds).

This module is also where the GPU tests take the loss, the pseudo-target and the rule from.
"""
import ctypes as C
import importlib

import numpy as np
import pytest

import fd_check as FD
import oracle_lib as O

CHARB_EPS = 0.05


def charbonnier_weights(H, W):
    """w(x, y) = 0 on the left third of the image, 1 + 0.5 sin(y / 5) elsewhere."""
    w = np.zeros((H, W), dtype=np.float64)
    y = np.arange(H, dtype=np.float64)
    x = np.arange(W)
    w[:, 3 * x >= W] = (1.0 + 0.5 * np.sin(y / 5.0))[:, None]
    return w


def charbonnier_terms(img, ref, w):
    """Per pixel and channel w * sqrt((C - ref)^2 + eps^2), in double."""
    d = img[..., :3].astype(np.float64) - ref[..., :3].astype(np.float64)
    return w[..., None] * np.sqrt(d * d + CHARB_EPS * CHARB_EPS)


def charbonnier_grad(img, ref, w):
    """dL/d(image0) of L = sum charbonnier_terms as an RGBA32F image (.w = 0): masked and signed."""
    d = img[..., :3].astype(np.float64) - ref[..., :3].astype(np.float64)
    g = np.zeros(img.shape, dtype=np.float32)
    g[..., :3] = (w[..., None] * d / np.sqrt(d * d + CHARB_EPS * CHARB_EPS)).astype(np.float32)
    return g


def pseudo_target(image0, g):
    """The target under which the reference's loss has (up to one fp32 rounding) the upstream gradient g at image0."""
    p = (image0.astype(np.float32) - g.astype(np.float32)).astype(np.float32)
    p[..., 3] = 1.0
    return p


def upstream_of(image0, pseudo):
    """fp32(image0 - pseudo): the bits the oracle's backward pass forms at main.cpp:616, which is what the GPU is given."""
    u = (image0.astype(np.float32) - pseudo.astype(np.float32)).astype(np.float32)
    u[..., 3] = 0.0
    return u


def check_general(render, loss_terms, analytic, splats9, which=None, rtol=1e-2, consist=4e-3):
    """fd_check.check for a general loss L = sum loss_terms(image) (an array per pixel and channel, in double): central
    differences at h and 2h per scalar, pairs whose two estimates disagree by more than `consist` are discontinuous on the
    interval and not used; the rest must agree with `analytic` within rtol; at least 60 % and at least 40 must be usable.
    L(+) - L(-) is summed term by term, so pixels the perturbed splat does not reach cancel exactly (fd_check.loss_delta)."""
    def central(i, k, h):
        base = np.float32(splats9[i, k])
        hi, lo = np.float32(base + np.float32(h)), np.float32(base - np.float32(h))
        s = splats9.copy()
        s[i, k] = hi
        tp = loss_terms(render(s))
        s[i, k] = lo
        tm = loss_terms(render(s))
        return float((tp - tm).sum()) / (float(hi) - float(lo))

    n = splats9.shape[0]
    which = range(n) if which is None else which
    scale = np.maximum(np.median(np.abs(analytic), axis=0), 1e-12)
    used, skipped, worst, worst_at = 0, 0, 0.0, None
    for i in which:
        for k in range(9):
            d1 = central(i, k, FD.STEPS[k])
            d2 = central(i, k, 2.0 * FD.STEPS[k])
            g = float(analytic[i, k])
            floor = 0.05 * scale[k]
            if abs(d1 - d2) > consist * max(abs(d1), abs(d2), floor):
                skipped += 1
                continue
            err = abs(g - d1) / max(abs(g), abs(d1), floor)
            used += 1
            if err > worst:
                worst, worst_at = err, (i, FD.NAMES[k], g, d1)
    stats = {"used": used, "skipped": skipped, "worst_rel": worst, "worst_at": worst_at}
    assert used >= 0.6 * (used + skipped) and used >= 40, stats
    assert worst <= rtol, stats
    return stats


class ExactOracle:
    """The oracle with expf on the fd_check scene: render(), and the backward pass from an upstream gradient."""

    def __init__(self, ref, n):
        self.o = O.OracleTrainer(ref, n)

    def render(self, s9):
        O.lib().s2do_set_exact_exp(1)
        try:
            self.o.splats[:] = np.ascontiguousarray(s9).view(O.SPLAT_DTYPE).reshape(-1)
            return self.o.forward().copy()
        finally:
            O.lib().s2do_set_exact_exp(0)

    def grads_from(self, s9, g):
        """-> (fp32 sums, dsum, dabs) of the backward pass at s9 whose dL/dC is fp32(image0 - pseudo_target(image0, g))."""
        img = self.render(s9)
        keep = self.o.ref
        O.lib().s2do_set_exact_exp(1)
        try:
            self.o.ref = np.ascontiguousarray(pseudo_target(img, g))
            w32, dsum, dabs = self.o.backward_stats()
            return w32.view(np.float32).reshape(-1, 9).copy(), dsum, dabs
        finally:
            self.o.ref = keep
            O.lib().s2do_set_exact_exp(0)


def test_device_pointer_entry_points_reject_null_arguments():
    """S2D_E_INVALID (1) for a null context or pointer, answered before any device call (this runs without a GPU)."""
    S2D = importlib.import_module("2dgaussiansplatting_amd")
    S2D._build.build_hip_library()
    lib = S2D.load_library()
    buf = (C.c_float * 16)()
    assert lib.s2d_backward_image_grads(None, buf, 0) == 1
    assert lib.s2d_backward_image_grads(None, None, 0) == 1
    assert lib.s2d_set_splats_device(None, buf) == 1
    assert lib.s2d_set_splats_device(None, None) == 1
    assert lib.s2d_get_image_rows_device(None, buf) == 1
    assert lib.s2d_get_image_rows_device(None, None) == 1
    for name in ("set_splats_device", "get_image_rows_device", "backward_image_grads"):
        assert callable(getattr(S2D.Trainer, name))


def test_pseudo_target_makes_the_oracle_differentiate_a_weighted_charbonnier_loss():
    s, ref = FD.scene()
    H, W = ref.shape[:2]
    w = charbonnier_weights(H, W)
    m = ExactOracle(ref, len(s))
    img = m.render(s)
    g = charbonnier_grad(img, ref, w)
    assert not g[:, : W // 3].any() and (g[..., :3] < 0).any() and (g[..., :3] > 0).any()  # masked, signed
    w32, dsum, dabs = m.grads_from(s, g)
    # what the oracle formed at main.cpp:616 is g to one rounding of the image's magnitude
    assert np.abs(upstream_of(img, pseudo_target(img, g)) - g).max() <= 2.0 ** -23
    st = check_general(m.render, lambda im: charbonnier_terms(im, ref, w), w32.astype(np.float64), s)
    print("\n[fd] oracle, expf, weighted Charbonnier through the pseudo-target: used %d skipped %d worst %.2e at %s"
          % (st["used"], st["skipped"], st["worst_rel"], st["worst_at"]))
    # the oracle's fp32 sums against the exact sum of the same terms
    nz = dabs > 0
    e = float((np.abs(w32 - dsum)[nz] / dabs[nz]).max())
    print("[fd] oracle fp32 sums vs exact: %.2e of sum |terms|; %d scalars with no term" % (e, int((~nz).sum())))
    assert e <= 1e-6
    # a splat wholly inside the masked third receives exactly nothing
    assert int((~nz).sum()) == 9 and np.all(w32[~nz] == 0)
    assert np.all((~nz).sum(axis=1) % 9 == 0)
