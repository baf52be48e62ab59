"""What the coverage tests share (tests/test_coverage_cpu.py, tests/test_gpu_coverage.py, tests/test_gpu_coverage_limits.py): the
three scenes, the white twin, the adversarial sweep, the reference's training loop with the fourth channel, the host program's
straight-alpha quantisation, and a float64 restatement of the four-channel blend with the exact exponential.

White twin: the same splats with their colours set to (1, 0, 0), in a plain context (or the oracle).  Its red channel is,
operation for operation, the coverage channel -- (T * 1) * alpha summed front to back -- and it comes out of kernels that the
oracle already pins."""
import functools
import os

import numpy as np

import oracle_lib as O

MINI = os.path.join(O.GOLDEN, "squirrel_cls_mini_268x213.s2di")
N_MINI = 2000
SCENES = ("mini", "tiny", "stack")


def white_twin(splats):
    """The splats (structured, or (n, 9) float32) with colour (1, 0, 0)."""
    s9 = np.array(np.asarray(splats).view(np.float32).reshape(-1, 9), dtype=np.float32, copy=True)
    s9[:, 5:8] = (1.0, 0.0, 0.0)
    return s9


def check_view_against_white_twin(vc, vp, vw, rgba8):
    """The white-twin yardstick for a view: vc, vp, vw are one view drawn by a coverage context, by a plain context with the same
    splats and by a plain context with their white twin.  The colours are the plain view's and the fourth channel is the
    twin's red, in bytes."""
    assert vc[..., :3].tobytes() == vp[..., :3].tobytes() and vp[..., :3].any()
    assert vc[..., 3].tobytes() == vw[..., 0].tobytes()
    assert len(np.unique(vc[..., 3])) > 1 and (vp[..., 3] == (255 if rgba8 else 1)).all()  # (a channel, not a constant)


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> (target RGBA32F with a non-trivial alpha, (n, 9) float32 splats), computed once and never written.
    mini:  the squirrel mini (268 x 213: partial tiles on both edges) with 2000 splats, the oracle advanced 3 steps, as
           tests/test_gpu_image_grads.py builds it;
    tiny:  17 x 17 with 40 small splats away from the top left corner: single-pixel partial tiles, untouched pixels;
    stack: 48 x 48 with a stack of 64 large splats of opacity 0.9: every pixel crosses the 1/256 cut-off, tile retirement runs,
           coverage sits just below 1."""
    if name == "mini":
        tgt = O.target_rgba32f(O.load_s2di(MINI))
        o = O.OracleTrainer(tgt, N_MINI)
        for _ in range(3):
            o.step()
        s9 = o.splats.view(np.float32).reshape(-1, 9).copy()
    elif name == "tiny":
        W = H = 17
        rng = np.random.default_rng(1717)
        n = 40
        s9 = np.zeros((n, 9), dtype=np.float32)
        s9[:, 0] = rng.uniform(6, W, n)  # (the top left corner stays empty: coverage exactly 0 there)
        s9[:, 1] = rng.uniform(6, H, n)
        s9[:, 2:4] = rng.uniform(0.5, 1.5, (n, 2))
        s9[:, 4] = rng.uniform(0, np.pi, n)
        s9[:, 5:8] = rng.uniform(0.1, 0.9, (n, 3))
        s9[:, 8] = rng.uniform(0.25, 0.95, n)
        tgt = O.synthetic_target(W, H)
    elif name == "stack":
        W = H = 48
        rng = np.random.default_rng(4848)
        n = 64
        s9 = np.zeros((n, 9), dtype=np.float32)
        s9[:, 0] = rng.uniform(16, 32, n)
        s9[:, 1] = rng.uniform(16, 32, n)
        s9[:, 2:4] = rng.uniform(60.0, 90.0, (n, 2))
        s9[:, 4] = rng.uniform(0, np.pi, n)
        s9[:, 5:8] = rng.uniform(0.1, 0.9, (n, 3))
        s9[:, 8] = 0.9
        tgt = O.synthetic_target(W, H)
    else:
        raise KeyError(name)
    tgt = tgt.copy()
    H, W = tgt.shape[:2]
    y, x = np.mgrid[0:H, 0:W]
    tgt[..., 3] = (0.5 + 0.5 * np.sin(x / 7.0) * np.cos(y / 5.0)).astype(np.float32)  # the alpha to fit: anything but a constant
    tgt.setflags(write=False)
    s9.setflags(write=False)
    return tgt, s9


def oracle_of(target, s9):
    o = O.OracleTrainer(np.ascontiguousarray(target), len(s9))
    o.splats.view(np.float32).reshape(-1, 9)[:] = s9
    return o


@functools.lru_cache(maxsize=None)
def oracle_frames(name):
    """-> (image0 of the scene, image0 of its white twin) from the oracle: the twin's red channel is the coverage."""
    tgt, s9 = scene(name)
    img = oracle_of(tgt, s9).forward().copy()
    twin = oracle_of(tgt, white_twin(s9)).forward().copy()
    img.setflags(write=False)
    twin.setflags(write=False)
    return img, twin


@functools.lru_cache(maxsize=None)
def assert_scenes_are_not_trivial():
    """Over the three scenes coverage has pixels that are exactly 0, pixels in (0.05, 0.95) and pixels above 0.99; the stack
    saturates (every pixel above 0.99 and none at 1: the cut-off stopped the walk) and the other two have partial tiles."""
    cov = {k: oracle_frames(k)[1][..., 0] for k in SCENES}
    allc = np.concatenate([c.ravel() for c in cov.values()])
    assert (allc == 0).any() and ((allc > 0.05) & (allc < 0.95)).any() and (allc > 0.99).any()
    assert (cov["stack"] > 0.99).all() and (cov["stack"] < 1.0).all()
    assert ((cov["tiny"] > 0.05) & (cov["tiny"] < 0.95)).any()
    assert ((cov["mini"] > 0.05) & (cov["mini"] < 0.95)).any()
    return True


def signed_upstream(H, W, seed=0):
    """A signed, spatially varying dL/dA, zero on the left third (the weights of tests/test_image_grads_cpu.py's Charbonnier
    construction times a sign pattern): (H, W) float32."""
    import test_image_grads_cpu as IG
    w = IG.charbonnier_weights(H, W)
    y, x = np.mgrid[0:H, 0:W]
    return (w * np.sin(0.37 * x + 0.23 * y + seed)).astype(np.float32)


def alpha_pattern(H, W):
    """The alpha to fit of the scenes and the sweep: anything but a constant, in [0, 1]."""
    y, x = np.mgrid[0:H, 0:W]
    return (0.5 + 0.5 * np.sin(x / 7.0) * np.cos(y / 5.0)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------
# the adversarial sweep
# ---------------------------------------------------------------------------------------------------------
SWEEP_SEEDS = range(24)
SWEEP_VARIANTS = ("plain", "generic_binning", "fp16_images", "deterministic")   # of seed % 4


@functools.lru_cache(maxsize=None)
def sweep_case(seed):
    """-> (W, H, n, splats, target_rgba), drawn as tests/test_gpu_parity.py::test_forward_and_gradients_random_sweep draws its
    cases: W in 1 .. 299, H in 1 .. 219 (down to one pixel, no tile multiples), n in {0, 1, 3, 40, 300, 700},
    oracle_lib.random_splats (thin, huge, rotated, off-centre), the synthetic target with alpha_pattern in .w.  Never written."""
    rng = np.random.default_rng(7000 + seed)
    W, H = int(rng.integers(1, 300)), int(rng.integers(1, 220))
    n = int(rng.choice([0, 1, 3, 40, 300, 700]))
    s = O.random_splats(n, W, H, 8000 + seed)
    tgt = O.synthetic_target(W, H)
    tgt[..., 3] = alpha_pattern(H, W)
    tgt.setflags(write=False)
    s.setflags(write=False)
    return W, H, n, s, tgt


def fp16_round(a):
    """float32 values rounded to binary16 and back: an image as a context with S2D_CFG_FP16_IMAGES stores it."""
    return np.asarray(a, dtype=np.float32).astype(np.float16).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------
# the reference's training loop with the fourth channel
# ---------------------------------------------------------------------------------------------------------
GEOM = [0, 1, 2, 3, 4, 8]   # pos.xy, sx, sy, rot, opacity: what the coverage reaches


class FourChannelOracle:
    """The reference's loop (forward, MSE, backward, Adam) for L = 1/2 sum (image0 - target)^2 over FOUR channels, out of two
    OracleTrainers and nothing else: the plain one differentiates the three colour channels against target.rgb, a white twin --
    the same splats coloured (1, 0, 0), whose red channel is the coverage A -- differentiates the fourth from the upstream
    (A - target.w, 0, 0, .), handed to it as a pseudo-target (tests/test_image_grads_cpu.py).  The gradient is the plain pass's
    nine columns plus the twin's geometric and opacity columns; the plain oracle's Adam step takes it.

    mode "f32": the two fp32 results added in fp32; "f64": the two passes' terms summed in double (dsum) added, rounded once.
    fp16: both frames and the target rounded to binary16 before the backward passes read them (S2D_CFG_FP16_IMAGES)."""

    def __init__(self, target_rgba, splats9, optimize_opacity=False, mode="f32", fp16=False):
        assert mode in ("f32", "f64")
        self.mode, self.fp16 = mode, bool(fp16)
        self.target = np.array(fp16_round(target_rgba) if fp16 else target_rgba, dtype=np.float32, copy=True)
        s9 = np.asarray(splats9).view(np.float32).reshape(-1, 9)
        self.n = len(s9)
        self.plain = O.OracleTrainer(self.target, self.n, optimize_opacity=optimize_opacity)
        self.twin = O.OracleTrainer(self.target, self.n)
        self.plain.splats.view(np.float32).reshape(-1, 9)[:] = s9
        self.coverage = None   # A of the last pass, (H, W) float32
        self.dabs = None       # summed |terms| of both passes of the last pass, (n, 9) float64

    @property
    def splats9(self):
        return self.plain.splats.view(np.float32).reshape(-1, 9)

    def gradients(self):
        """One forward and backward pass of both oracles on the current splats -> (mse, g32 (n, 9) float32 in the chosen mode,
        dsum (n, 9) float64: all terms of both passes summed in double); self.dabs, self.coverage as described."""
        import test_image_grads_cpu as IG
        p, w = self.plain, self.twin
        p.ref = self.target
        p.forward()
        if self.fp16:
            p.image0[:] = fp16_round(p.image0)
        mse = p.mse()
        d_p, dsum_p, dabs_p = p.backward_stats()
        w.splats.view(np.float32).reshape(-1, 9)[:] = white_twin(p.splats)
        w.forward()
        if self.fp16:
            w.image0[:] = fp16_round(w.image0)
        self.coverage = w.image0[..., 0].copy()
        gu = np.zeros(w.image0.shape, dtype=np.float32)
        gu[..., 0] = self.coverage - self.target[..., 3]
        w.ref = np.ascontiguousarray(IG.pseudo_target(w.image0, gu))
        d_w, dsum_w, dabs_w = w.backward_stats()
        g32 = d_p.view(np.float32).reshape(-1, 9).copy()
        dsum, dabs = dsum_p.copy(), dabs_p.copy()
        dsum[:, GEOM] += dsum_w[:, GEOM]
        dabs[:, GEOM] += dabs_w[:, GEOM]
        if self.mode == "f32":
            g32[:, GEOM] += d_w.view(np.float32).reshape(-1, 9)[:, GEOM]
        else:
            g32 = dsum.astype(np.float32)
        self.dabs = dabs
        return mse, g32, dsum

    def step(self, lr=0.05):
        """One iteration -> (status of the Adam step, the MSE the reference prints: three channels, before the step)."""
        mse, g32, _ = self.gradients()
        self.plain.dsplats.view(np.float32).reshape(-1, 9)[:] = g32
        st = self.plain.adam(lr)
        self.plain.iterations += 1
        return st, mse

    def run(self, iters):
        """-> (the per-iteration MSEs, the summed |terms| of both passes of the last iteration)."""
        out = []
        for _ in range(iters):
            st, mse = self.step()
            assert st == 0
            out.append(mse)
        return np.array(out), self.dabs


@functools.lru_cache(maxsize=None)
def five_steps(name, opacity, mode="f32"):
    """FourChannelOracle on a scene, five iterations, once -> (MSEs, (n, 9) float64 parameters afterwards)."""
    tgt, s9 = scene(name)
    o = FourChannelOracle(tgt, s9, optimize_opacity=opacity, mode=mode)
    mse, _ = o.run(5)
    sp = o.splats9.astype(np.float64)
    mse.setflags(write=False)
    sp.setflags(write=False)
    return mse, sp


def update_bar(ref, steps=5, lr=0.05):
    """The bar of tests/test_gpu_parity.py::test_training_steps_random_sweep on parameters after `steps` iterations."""
    return steps * 1e-3 * lr + 1e-5 * float(np.abs(ref).max())


# ---------------------------------------------------------------------------------------------------------
# the host program's RGBA8 output
# ---------------------------------------------------------------------------------------------------------
def straight_rgba8(image0):
    """s2dio::quantise_straight (host/image_io.h) in NumPy, fp32 throughout: (premultiplied colour, coverage) -> RGBA8 with
    straight alpha.  c / a where a > 0, otherwise 0; v * 255 + 0.5 clamped to [0, 255] and truncated; alpha byte 0 where
    a <= 0."""
    f = np.ascontiguousarray(image0, dtype=np.float32)
    a = f[..., 3]
    pos = a > 0

    def q(v):
        v = v * np.float32(255.0) + np.float32(0.5)
        return np.where(v < 0, np.float32(0), np.where(v > 255, np.float32(255), v)).astype(np.uint8)

    out = np.zeros(f.shape, dtype=np.uint8)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        ratio = f[..., :3] / np.where(pos, a, np.float32(1.0))[..., None]
        out[..., :3] = np.where(pos[..., None], q(ratio), 0)
        out[..., 3] = np.where(pos, q(a), 0)
    return out


# ---------------------------------------------------------------------------------------------------------
# float64 restatement of the four-channel blend (exact exponential), for the finite-difference test
# ---------------------------------------------------------------------------------------------------------
def inv_cov(sx, sy, th):
    c, s = np.cos(th), np.sin(th)
    l0, l1 = sx * sx, sy * sy
    s11 = l0 * c * c + l1 * s * s
    s12 = (l0 - l1) * s * c
    s22 = l0 + l1 - s11
    det = s11 * s22 - s12 * s12
    return s22 / det, -s12 / det, s11 / det


def alphas_of(s9, W, H):
    """(n, H, W) float64: alpha of every splat at every pixel centre, every pixel visited, no cut-off."""
    y, x = np.mgrid[0:H, 0:W]
    out = np.zeros((len(s9), H, W))
    for i, r in enumerate(np.asarray(s9, dtype=np.float64)):
        a, b, d = inv_cov(r[2], r[3], r[4])
        vx, vy = x + 0.5 - r[0], y + 0.5 - r[1]
        out[i] = r[8] * np.exp(-0.5 * (vx * (a * vx + b * vy) + vy * (b * vx + d * vy)))
    return out


def coverage_of(s9, W, H):
    """A = sum_i T_i alpha_i, the fourth channel: (H, W) float64."""
    T, A = np.ones((H, W)), np.zeros((H, W))
    for al in alphas_of(s9, W, H):
        A = A + T * al
        T = T * (1.0 - al)
    return A


def coverage_grads(s9, W, H, w):
    """Analytic d(sum w * A)/d(pos.xy, sx, sy, rot, opacity) as the backward walk forms it: per (pixel, splat) the alpha
    derivative of the coverage is T - S_a / (1 - alpha) with S_a = A_final - A_running (main.cpp:627-628 for c = 1), times the
    reference's d alpha / d parameter (main.cpp:639-640, :657-662, :680-683, :703).  -> (n, 9) float64, colour columns 0."""
    s = np.asarray(s9, dtype=np.float64)
    al = alphas_of(s, W, H)
    A = coverage_of(s, W, H)
    y, x = np.mgrid[0:H, 0:W]
    g = np.zeros((len(s), 9))
    T, run = np.ones((H, W)), np.zeros((H, W))
    for i, r in enumerate(s):
        a, b, d = inv_cov(r[2], r[3], r[4])
        vx, vy = x + 0.5 - r[0], y + 0.5 - r[1]
        run = run + T * al[i]
        dA_dalpha = T - (A - run) / (1.0 - al[i])
        gs = w * dA_dalpha
        ga = gs * al[i]
        cos, sin = np.cos(r[4]), np.sin(r[4])
        g[i, 0] = np.sum(ga * (a * vx + b * vy))
        g[i, 1] = np.sum(ga * (b * vx + d * vy))
        g[i, 2] = np.sum(ga / r[2] ** 3 * (cos * cos * vx * vx + 2 * sin * cos * vx * vy + sin * sin * vy * vy))
        g[i, 3] = np.sum(ga / r[3] ** 3 * (sin * sin * vx * vx - 2 * sin * cos * vx * vy + cos * cos * vy * vy))
        g[i, 4] = np.sum(ga * (r[2] ** 2 - r[3] ** 2) / (r[2] ** 2 * r[3] ** 2) *
                         ((cos * cos - sin * sin) * vx * vy - sin * cos * (vx * vx - vy * vy)))
        g[i, 8] = np.sum(gs * al[i] / r[8])
        T = T * (1.0 - al[i])
    return g
