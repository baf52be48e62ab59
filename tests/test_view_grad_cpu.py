"""CPU tests of the backward pass through a view (include/splat2d.h "view gradients"):
  * view_row_adjoint of csrc/s2d_view_math.h, compiled for the host, against the NumPy restatement tests/view_grad_ref.py in
    BYTES;
  * that restatement in float64 against central differences of the record transform in float64, under the bars of
    tests/fd_check.py as they stand;
  * the adjoint of the resolve against the resolve;
  * the binding lists the two entry points;
  * the finite-difference yardstick of the operator's GPU test, on the oracle alone."""
import importlib

import numpy as np
import pytest

import fd_check as FD
import oracle_lib as O
import test_image_grads_cpu as IG
import view_grad_hostcheck
import view_grad_ref as G
import view_ref as V

F = np.float32


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fv", [0.0, 0.75], ids=["nofilter", "filter"])
@pytest.mark.parametrize("samples", [1, 2, 4])
@pytest.mark.parametrize("view", V.VIEWS, ids=V.VIEW_IDS)
def test_host_adjoint_equals_the_restatement_in_bytes(view, samples, fv):
    L = view_grad_hostcheck.load()
    origin, zoom, _, _ = view
    s9 = np.ascontiguousarray(G.rows9(V.scene_m()))
    g = G.random_record_grads(len(s9), seed=samples)
    assert (g < 0).any() and (g == 0).any() and not g[::7].any()
    got = np.full_like(g, np.nan)
    L.vgc_adjoint(O._p(s9), O._p(g), len(s9), origin[0], origin[1], zoom, fv, samples, O._p(got))
    want = G.adjoint(s9, g, origin, zoom, fv, samples)
    assert want.dtype == np.float32 and np.isfinite(want).all()
    assert got.tobytes() == want.tobytes()
    assert not got[::7].any()   # a zero gradient stays zero
    if fv:                      # the filter couples the opacity gradient into the scales
        assert np.any(got[:, 2] != g[:, 2] * (F(zoom) * F(samples)))


def test_samples_zero_means_one():
    L = view_grad_hostcheck.load()
    s9 = np.ascontiguousarray(G.rows9(V.scene_m()))
    g = G.random_record_grads(len(s9))
    a, b = np.empty_like(g), np.empty_like(g)
    L.vgc_adjoint(O._p(s9), O._p(g), len(s9), 1.0, 2.0, 0.5, 0.75, 0, O._p(a))
    L.vgc_adjoint(O._p(s9), O._p(g), len(s9), 1.0, 2.0, 0.5, 0.75, 1, O._p(b))
    assert a.tobytes() == b.tobytes()


# 2 ---------------------------------------------------------------------------------------------------------------------------
# (origin, zoom, filter_var, samples); the last two: fr = filter_var * s^2 dominates ax^2 = (sx * zoom * s)^2 for the 2-pixel scales
FD_CASES = [((5.25, 3.5), 2.5, 0.0, 1), ((0.0, 0.0), 0.5, 0.75, 2), ((0.0, 0.0), 0.05, 6.0, 1), ((3.0, -2.0), 0.02, 40.0, 4)]


@pytest.mark.parametrize("case", FD_CASES, ids=["nofilter", "v3_s2", "filter_dominates", "filter_dominates_s4"])
def test_float64_adjoint_is_the_derivative_of_the_record_transform(case):
    """The scalar function is <g', view_rows(p)>: its gradient with respect to p is adjoint(p, g').  Central differences at
    fd_check's steps h and 2h; fd_check.check's rule and thresholds (consist 4e-3, rtol 1e-2, at least 60 % and 40 used)."""
    origin, zoom, fv, samples = case
    p = G.rows9(V.scene_m())[:24].astype(np.float64)
    g = G.random_record_grads(len(p), seed=5).astype(np.float64)
    if fv:
        ax = p[:, 2] * zoom * samples
        assert ((fv * samples * samples > ax * ax).any()) == (zoom < 0.1)
    analytic = G.adjoint(p, g, origin, zoom, fv, samples, dtype=np.float64)

    def f(q):
        return float((g * G.view_rows9(q, origin, zoom, fv, samples)).sum())

    scale = np.maximum(np.median(np.abs(analytic), axis=0), 1e-12)
    used, skipped, worst = 0, 0, 0.0
    for i in range(len(p)):
        for k in range(9):
            d = []
            for h in (FD.STEPS[k], 2.0 * FD.STEPS[k]):
                hi, lo = p.copy(), p.copy()
                hi[i, k] += h
                lo[i, k] -= h
                d.append((f(hi) - f(lo)) / (hi[i, k] - lo[i, k]))
            floor = 0.05 * scale[k]
            if abs(d[0] - d[1]) > 4e-3 * max(abs(d[0]), abs(d[1]), floor):
                skipped += 1
                continue
            used += 1
            worst = max(worst, abs(analytic[i, k] - d[0]) / max(abs(analytic[i, k]), abs(d[0]), floor))
    assert used >= 0.6 * (used + skipped) and used >= 40, (used, skipped)
    assert worst <= 1e-2, worst


# 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("samples", [2, 4])
def test_expand_is_the_adjoint_of_the_resolve(samples):
    rng = np.random.default_rng(samples)
    h, w = 6, 10
    img = rng.uniform(-1, 1, (h * samples, w * samples, 3))
    u = rng.uniform(-1, 1, (h, w, 3))
    lhs = float((G.resolve64(img, samples) * u).sum())
    rhs = float((img * G.expand(u, samples)).sum())
    assert abs(lhs - rhs) <= 1e-13 * float(np.abs(img).sum())
    # in float32 the expansion is exact: the same bits as the float64 one
    u32 = u.astype(F)
    assert G.expand(u32, samples).dtype == F
    assert np.array_equal(G.expand(u32, samples).astype(np.float64), G.expand(u32.astype(np.float64), samples))
    assert G.expand(u32, 1).tobytes() == u32.tobytes()


# 4 ---------------------------------------------------------------------------------------------------------------------------
def test_binding_lists_the_entry_points():
    S2D = importlib.import_module("2dgaussiansplatting_amd")
    assert "s2d_view_backward_device" in S2D.ABI_SYMBOLS and "s2d_view_grads" in S2D.ABI_SYMBOLS
    assert S2D.S2D_VIEW_BWD_FROM_TARGET == 0x8
    for name in ("view_backward_device", "view_grads"):
        assert callable(getattr(S2D.Trainer, name))
    S2D._build.build_hip_library()
    lib = S2D.load_library()
    assert lib.s2d_view_backward_device(None, None, None, 0) == 1   # S2D_E_INVALID before any device work
    assert lib.s2d_view_grads(None, None, None, 0, None) == 1


# 5 ---------------------------------------------------------------------------------------------------------------------------
class OracleView:
    """The view of tests/view_grad_ref.py FD_VIEW with none of the library's code: the oracle's forward loop (expf) on the NumPy
    records at the grid size, NumPy's resolve; its backward pass from the expanded weights (pseudo-target method), NumPy's
    adjoint."""

    def __init__(self, n, ow, oh):
        self.ow, self.oh, self.S = ow, oh, G.FD_VIEW["samples"]
        self.o = O.OracleTrainer(O.synthetic_target(ow * self.S, oh * self.S), n)

    def grid(self, s9):
        v = G.FD_VIEW
        rows = V.view_rows(np.ascontiguousarray(s9).view(O.SPLAT_DTYPE).reshape(-1), v["origin"], v["zoom"], v["filter_var"], self.S)
        O.lib().s2do_set_exact_exp(1)
        try:
            self.o.splats[:] = rows
            return self.o.forward().copy()
        finally:
            O.lib().s2do_set_exact_exp(0)

    def render(self, s9):
        return V.resolve(self.grid(s9), self.S)

    def grads(self, s9, w3):
        v = G.FD_VIEW
        img = self.grid(s9)
        up = np.zeros((self.oh, self.ow, 4), dtype=F)
        up[..., :3] = w3
        O.lib().s2do_set_exact_exp(1)
        try:
            self.o.ref = np.ascontiguousarray(IG.pseudo_target(img, G.expand(up, self.S)))
            w32 = self.o.backward_stats()[0].view(np.float32).reshape(-1, 9).astype(np.float64)
        finally:
            O.lib().s2do_set_exact_exp(0)
        return G.adjoint(np.asarray(s9, dtype=np.float64), w32, v["origin"], v["zoom"], v["filter_var"], self.S, dtype=np.float64)


def test_the_operator_fd_yardstick_holds_on_the_oracle_alone():
    """What tests/test_gpu_view_grad.py::test_operator_view_backward_is_the_derivative asks of the operator is asked here of
    the oracle, so that a miss there is the operator's: same scene, view, weights, steps and bars (check_general unchanged).
    The weights are view_grad_ref.fd_weights.  Two other choices were measured on this oracle chain and are NOT usable, because
    the yardstick itself misses its 1e-2 with them under view 3's low-pass: weights 1 + 0.5 sin(y / 5) with a masked third
    (worst 2.14e-2 at (splat 2, rot): analytic 0.0667905 against 0.0653611; the differences at 8 and 32 times the step give
    0.066926 and 0.066769) and view - target held fixed (1.16e-2 at (splat 4, rot)); with these weights the rot derivatives are
    small residues and the loss moves by ~3e-5 at fd_check's rot step against ~4e-7 of fp32 noise in the forward pass."""
    s, ref = FD.scene()
    oh, ow = ref.shape[0] // 2, ref.shape[1] // 2
    m = OracleView(len(s), ow, oh)
    w3 = G.fd_weights(m.render(s), G.box_half(ref), IG.charbonnier_grad, IG.charbonnier_weights)
    assert (w3 < 0).any() and (w3 > 0).any() and not w3[:, : ow // 3].any()
    st = IG.check_general(m.render, lambda im: w3.astype(np.float64) * im[..., :3].astype(np.float64), m.grads(s, w3), s)
    print("\n[fd] oracle view, expf, view 3 x 2: used %d skipped %d worst %.2e at %s" % (st["used"], st["skipped"], st["worst_rel"], st["worst_at"]))
