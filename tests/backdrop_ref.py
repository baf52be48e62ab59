"""What the backdrop tests share (tests/test_backdrop_cpu.py, tests/test_gpu_backdrop.py; include/splat2d_backdrop.h, DESIGN.md
section 25): the oracle over a backdrop, the scenes, and a float64 restatement of the composite and of the backward walk's
expression for the finite-difference test.  A helper, not a test module.

BackdropOracle wraps oracle_lib.OracleTrainer and needs no new C: the oracle's backward pass leaves T_final in image1[..., 3],
formed by the forward loop's own operations, and takes image0 as an argument.  One pass is
  forward()                                  C into image0
  backward()                                 only to read T = image1[..., 3]  (its gradients are thrown away)
  image0.rgb = image0.rgb + T * B            NumPy float32, the multiply first
  backward_stats() on that image0, adam()
With fp16 images the target and image0 are rounded to binary16 and back, the rule of tests/test_gpu_parity.py (_fp16)."""
import functools

import numpy as np

import coverage_ref as CR
import oracle_lib as O

F32 = np.float32


def fp16_round(a):
    return np.asarray(a, dtype=F32).astype(np.float16).astype(F32)


def composite(plain, T, backdrop):
    """image0 of a backdrop context from the plain framebuffer, T_final (H, W) and the backdrop ((3,) or (H, W, 4)): float32,
    one multiply, then one add; .w stays as it is."""
    out = np.array(plain, dtype=F32, copy=True)
    B = np.asarray(backdrop, dtype=F32)
    Brgb = B if B.ndim == 1 else B[..., :3]
    T = np.asarray(T, dtype=F32)
    prod = (T[..., None] * Brgb).astype(F32)
    out[..., :3] = (out[..., :3] + prod).astype(F32)
    return out


class BackdropOracle:
    def __init__(self, target, splats, backdrop, optimize_opacity=False, fp16=False):
        """splats: structured or (n, 9) float32, or an int n (the oracle's init())."""
        self.fp16 = bool(fp16)
        tgt = np.array(fp16_round(target) if fp16 else target, dtype=F32, copy=True)
        if isinstance(splats, (int, np.integer)):
            self.o = O.OracleTrainer(tgt, int(splats), optimize_opacity=optimize_opacity)
        else:
            s9 = np.asarray(splats).view(F32).reshape(-1, 9)
            self.o = O.OracleTrainer(tgt, len(s9), optimize_opacity=optimize_opacity)
            self.o.splats.view(F32).reshape(-1, 9)[:] = s9
        self.backdrop = np.array(backdrop, dtype=F32, copy=True)
        self.T = None

    @property
    def splats9(self):
        return self.o.splats.view(F32).reshape(-1, 9)

    def forward(self):
        """-> image0 over the backdrop (also left in the oracle's image0); self.T = T_final (H, W) float32."""
        o = self.o
        o.forward()
        o.backward()
        self.T = o.image1[..., 3].copy()
        img = composite(o.image0, self.T, self.backdrop)
        if self.fp16:
            img = fp16_round(img)
        o.image0[:] = img
        return o.image0

    def backward_stats(self):
        """The oracle's backward pass on the composite -> (fp32 gradients, dsum, dabs)."""
        return self.o.backward_stats()

    def step(self):
        """One iteration -> (status of the Adam step, the MSE of the composite before the step)."""
        self.forward()
        mse = self.o.mse()
        self.o.backward_stats()
        st = self.o.adam()
        self.o.iterations += 1
        return st, mse


# ---------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------
def noise_plane(W, H, seed=5):
    """An (H, W, 4) float32 plane backdrop: noise in [0, 1] in the colours, junk in .w (it is ignored)."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.0, 1.0, (H, W, 4)).astype(F32)
    p[..., 3] = rng.uniform(-5.0, 5.0, (H, W)).astype(F32)
    return p


CONSTANT = np.array([1.0, 0.5, 0.25], dtype=F32)
SCENES = ("tiny", "stack", "deep", "ones", "empty", "row")


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> (target RGBA32F, (n, 9) float32 splats), never written.
    tiny:  17 x 17, 40 small splats, the top left corner untouched (T_final exactly 1 there): partial tiles, an empty wave;
    stack: 48 x 48, 64 large splats of opacity 0.9: every pixel crosses the 1/256 cut-off and every tile retires early;
    deep:  64 x 48, 600 low-opacity splats: several entry batches per tile, T small but above the cut-off for long;
    ones:  48 x 32, minimum-size splats of opacity 1 on pixel centres, corners and borders: T_final exactly 0 at a centre;
    empty: 40 x 24 without splats; row: 200 x 1 with 50 splats; wide: 300 x 230 with three splats (69000 pixels: more than one
    stride of the gradient kernel's 256 workgroups of 256 threads)."""
    if name in ("tiny", "stack"):
        tgt, s9 = CR.scene(name)
        tgt = np.array(tgt, copy=True)
        tgt[..., 3] = 1.0
        s9 = np.array(s9, copy=True)
    elif name == "deep":
        W, H, n = 64, 48, 600
        rng = np.random.default_rng(22)
        s = np.zeros(n, dtype=O.SPLAT_DTYPE)
        s["pos"][:, 0] = rng.uniform(0, W - 1, n)
        s["pos"][:, 1] = rng.uniform(0, H - 1, n)
        s["sx"] = rng.uniform(4, 12, n)
        s["sy"] = rng.uniform(4, 12, n)
        s["rot"] = rng.uniform(0, np.pi, n)
        s["color"] = rng.uniform(0, 1, (n, 3))
        s["opacity"] = rng.choice([0.1, 0.15, 0.3], n)
        tgt, s9 = O.synthetic_target(W, H), s.view(F32).reshape(-1, 9).copy()
    elif name == "ones":
        W, H = 48, 32
        pts = [(x + dx, y + dy) for x in (0, 15, 16, 31, 47) for y in (0, 15, 16, 31) for dx, dy in ((0.5, 0.5), (0.0, 0.0))]
        pts = [(min(px, W - 1), min(py, H - 1)) for px, py in pts]
        n = len(pts)
        s = np.zeros(n, dtype=O.SPLAT_DTYPE)
        s["pos"] = np.array(pts, dtype=F32)
        s["sx"] = 1.0
        s["sy"] = 1.0
        s["rot"] = np.linspace(0, 3, n)
        s["color"] = np.linspace(0.1, 0.9, n)[:, None]
        s["opacity"] = 1.0
        tgt, s9 = O.synthetic_target(W, H), s.view(F32).reshape(-1, 9).copy()
    elif name == "empty":
        tgt, s9 = O.synthetic_target(40, 24), np.zeros((0, 9), dtype=F32)
    elif name == "row":
        W, H = 200, 1
        s = O.random_splats(50, W, 4, 31)
        s["pos"][:, 1] = 0
        tgt, s9 = O.synthetic_target(W, H), s.view(F32).reshape(-1, 9).copy()
    elif name == "wide":
        W, H = 300, 230
        tgt, s9 = O.synthetic_target(W, H), O.random_splats(3, W, H, 77).view(F32).reshape(-1, 9).copy()
    else:
        raise KeyError(name)
    tgt.setflags(write=False)
    s9.setflags(write=False)
    return tgt, s9


SWEEP_SEEDS = range(12)
SWEEP_VARIANTS = ("plain", "generic_binning", "fp16_images", "deterministic")   # of seed % 4


@functools.lru_cache(maxsize=None)
def sweep_case(seed):
    """-> (W, H, n, splats, target): W in 36 .. 289, H in 20 .. 150, n in {1, 3, 40, 300, 700}, oracle_lib.random_splats."""
    rng = np.random.default_rng(9100 + seed)
    W, H = int(rng.integers(36, 290)), int(rng.integers(20, 151))
    n = int(rng.choice([1, 3, 40, 300, 700]))
    s = O.random_splats(n, W, H, 9200 + seed)
    tgt = O.synthetic_target(W, H)
    tgt.setflags(write=False)
    s.setflags(write=False)
    return W, H, n, s, tgt


@functools.lru_cache(maxsize=None)
def reference(name, kind, fp16=False):
    """BackdropOracle's forward and backward pass on a scene, once -> (image0, T, fp32 gradients (n, 9), dsum, dabs), never written.
    kind: "constant" (CONSTANT) or "plane" (noise_plane of the scene's size)."""
    tgt, s9 = scene(name)
    H, W = tgt.shape[:2]
    b = BackdropOracle(tgt, s9, CONSTANT if kind == "constant" else noise_plane(W, H), fp16=fp16)
    img = b.forward().copy()
    w32, dsum, dabs = b.backward_stats()
    out = (img, b.T.copy(), w32.view(F32).reshape(-1, 9).copy(), dsum.copy(), dabs.copy())
    for a in out:
        a.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------------
# float64 restatement of the composite (exact exponential, no cut-off), for the finite-difference test
# ---------------------------------------------------------------------------------------------------------
def composite_of(s9, W, H, backdrop):
    """I = sum_i c_i T_i alpha_i + T_final * B: (H, W, 3) float64.  backdrop: (3,) or (H, W, 3)."""
    s = np.asarray(s9, dtype=np.float64)
    T, I = np.ones((H, W)), np.zeros((H, W, 3))
    for i, al in enumerate(CR.alphas_of(s, W, H)):
        I = I + (T * al)[..., None] * s[i, 5:8]
        T = T * (1.0 - al)
    return I + T[..., None] * np.asarray(backdrop, dtype=np.float64)


def composite_grads(s9, W, H, w, backdrop):
    """Analytic d(sum w * I)/d(splat), w (H, W, 3), as the backward walk forms it with the composite in the place of the final
    colour: per (pixel, splat, channel) the alpha derivative is c_i T_i - S / (1 - alpha_i), S = I_final - I_running
    (main.cpp:627-628), where I_final carries the backdrop's share T_final * B; times the reference's d alpha / d parameter.
    The colour derivative is T_i alpha_i.  -> (n, 9) float64."""
    s = np.asarray(s9, dtype=np.float64)
    al = CR.alphas_of(s, W, H)
    fin = composite_of(s, W, H, backdrop)
    y, x = np.mgrid[0:H, 0:W]
    g = np.zeros((len(s), 9))
    T, run = np.ones((H, W)), np.zeros((H, W, 3))
    for i, r in enumerate(s):
        a, b, d = CR.inv_cov(r[2], r[3], r[4])
        vx, vy = x + 0.5 - r[0], y + 0.5 - r[1]
        run = run + (T * al[i])[..., None] * r[5:8]
        dI_dalpha = T[..., None] * r[5:8] - (fin - run) / (1.0 - al[i])[..., None]
        gs = np.sum(w * dI_dalpha, axis=-1)
        ga = gs * al[i]
        cos, sin = np.cos(r[4]), np.sin(r[4])
        g[i, 0] = np.sum(ga * (a * vx + b * vy))
        g[i, 1] = np.sum(ga * (b * vx + d * vy))
        g[i, 2] = np.sum(ga / r[2] ** 3 * (cos * cos * vx * vx + 2 * sin * cos * vx * vy + sin * sin * vy * vy))
        g[i, 3] = np.sum(ga / r[3] ** 3 * (sin * sin * vx * vx - 2 * sin * cos * vx * vy + cos * cos * vy * vy))
        g[i, 4] = np.sum(ga * (r[2] ** 2 - r[3] ** 2) / (r[2] ** 2 * r[3] ** 2) *
                         ((cos * cos - sin * sin) * vx * vy - sin * cos * (vx * vx - vy * vy)))
        g[i, 5:8] = np.sum(w * (T * al[i])[..., None], axis=(0, 1))
        g[i, 8] = np.sum(gs * al[i] / r[8])
        T = T * (1.0 - al[i])
    return g


def backdrop_grads_of(s9, W, H, w):
    """d(sum w * I)/dB: per pixel and channel T_final * w -> (H, W, 3) float64."""
    T = np.ones((H, W))
    for al in CR.alphas_of(np.asarray(s9, dtype=np.float64), W, H):
        T = T * (1.0 - al)
    return T[..., None] * w


# ---------------------------------------------------------------------------------------------------------
# the squared error (main.cpp:796-805) and when its sum does not depend on the order
# ---------------------------------------------------------------------------------------------------------
def sqerr_terms(image0, target):
    """lengthSquared((image0 - target).rgb * 255) per pixel as the reference forms it: a float32 per pixel."""
    d = ((np.asarray(image0, dtype=F32)[..., :3] - np.asarray(target, dtype=F32)[..., :3]).astype(F32) * F32(255.0)).astype(F32)
    sq = (d * d).astype(F32)
    return ((sq[..., 0] + sq[..., 1]).astype(F32) + sq[..., 2]).astype(F32)


def sum_is_order_free(terms):
    """True when the double sum of these non-negative float32 terms is exact in EVERY order: all terms are multiples of 2^q (q from
    the smallest term's last mantissa bit) and the total stays below 2^(53 + q), so every partial sum of every order is a multiple
    of 2^q below 2^(53 + q) and therefore a double.  Then the GPU's tile-wise sum and the oracle's row-wise sum are the same
    number and their quotients by 3 W H the same double."""
    t = np.asarray(terms, dtype=np.float64).ravel()
    nz = t[t > 0]
    if len(nz) == 0:
        return True
    _, e = np.frexp(nz)          # nz = m * 2^e with m in [0.5, 1): a float32's last bit is 2^(e - 24)
    q = int((e - 24).min())
    return bool(float(np.sum(nz)) < 2.0 ** (53 + q))
