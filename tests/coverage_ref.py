"""What the coverage tests share (tests/test_coverage_cpu.py, tests/test_gpu_coverage.py): the three scenes, the white twin, and
a float64 restatement of the four-channel blend with the exact exponential.

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
