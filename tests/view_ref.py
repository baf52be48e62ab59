"""NumPy restatement of view rendering (include/splat2d.h, s2d_view_config; csrc/s2d_view_math.h): the record transform, the
supersampling resolve, the 8-bit quantiser and the refusal table, plus the scenes and views the tests share.  Every float
expression is a chain of single fp32 operations in the order the header states."""
import ctypes as C

import numpy as np

import oracle_lib as O

F = np.float32

# (origin, zoom, filter_var, (out_width, out_height)) -- on scene M (64 x 48) all six keep the transformed scales in [1, 1024]
VIEWS = [
    ((5.25, 3.5), 2.5, 0.0, (53, 37)),     # 1: output not a multiple of 16
    ((0.0, 0.0), 0.5, 0.0, (32, 24)),      # 2: minification
    ((0.0, 0.0), 0.5, 0.75, (32, 24)),     # 3: minification with the low-pass
    ((-4.0, -4.0), 1.0, 0.0, (72, 56)),    # 4: a border outside the source
    ((16.0, 16.0), 1.0, 0.0, (32, 16)),    # 5: an integer crop
    ((20.0, 10.0), 16.0, 0.0, (160, 96)),  # 6: large zoom
]
VIEW_IDS = ["v%d" % (k + 1) for k in range(len(VIEWS))]
SRC_W, SRC_H, N_SPLATS = 64, 48, 600


def scene_m():
    """Source 64 x 48, n = 600: every tile's list spans several 64-entry batches."""
    rng = np.random.default_rng(7)
    s = np.zeros(N_SPLATS, dtype=O.SPLAT_DTYPE)
    s["pos"][:, 0] = rng.uniform(0, SRC_W - 1, N_SPLATS)
    s["pos"][:, 1] = rng.uniform(0, SRC_H - 1, N_SPLATS)
    s["sx"] = rng.choice([2.0, 3.0, 6.0, 12.0, 40.0], N_SPLATS)
    s["sy"] = rng.choice([2.0, 2.5, 5.0, 9.0, 30.0], N_SPLATS)
    s["rot"] = rng.uniform(-7, 7, N_SPLATS)
    s["color"] = rng.uniform(0, 1, (N_SPLATS, 3))
    s["opacity"] = rng.uniform(0.1, 1.0, N_SPLATS)
    return s


def scene_a(seed=11):
    return O.random_splats(N_SPLATS, SRC_W, SRC_H, seed)


# The short end of the tile lists: scene M's splats shrunk to sx = sy = 2 (as test_far_border_is_background shrinks them), the
# top left corner of the source at zoom 4 with a border outside it.  At 1, 2 and 4 samples per axis the raster grid (75 x 53,
# 150 x 106, 300 x 212: partial tiles) has tiles whose lists are empty, hold exactly one entry, fewer than 32 and between 33
# and 63 -- no list reaches a staging batch of 64 (from the footprints' rectangles: at most 43, 42, 39 entries); the
# transformed scales are 8, 16 and 32.  tests/test_gpu_view_variants.py asserts all of it on the lists the library builds.
SPARSE_VIEW = ((-9.5, -7.5), 4.0, 0.0, (75, 53))


def scene_sparse():
    s = scene_m()
    s["sx"], s["sy"] = 2.0, 2.0
    return s


def view_rows(splats, origin, zoom, filter_var=0.0, samples=1):
    """The records a view rasterises."""
    s = 1 if samples == 0 else int(samples)
    zr = F(zoom) * F(s)
    fr = F(filter_var) * F(s * s)
    out = np.array(splats, dtype=O.SPLAT_DTYPE, copy=True)
    with np.errstate(all="ignore"):
        out["pos"][:, 0] = (splats["pos"][:, 0] - F(origin[0])) * zr
        out["pos"][:, 1] = (splats["pos"][:, 1] - F(origin[1])) * zr
        ax = splats["sx"] * zr
        ay = splats["sy"] * zr
        if fr == 0:
            out["sx"], out["sy"] = ax, ay
        else:
            sx = np.sqrt(ax * ax + fr)
            sy = np.sqrt(ay * ay + fr)
            out["sx"], out["sy"] = sx, sy
            out["opacity"] = splats["opacity"] * ((ax * ay) / (sx * sy))
    return out


def scales_in_pinned_range(rows):
    """The range of scales the parity tests pin the rasteriser to the oracle on."""
    return bool(np.all((rows["sx"] >= 1) & (rows["sx"] <= 1024) & (rows["sy"] >= 1) & (rows["sy"] <= 1024)))


def resolve2(img):
    """One level: ((p00 + p01) + (p10 + p11)) * 0.25f per channel; .w = 1."""
    img = np.asarray(img, dtype=F)
    with np.errstate(all="ignore"):
        out = ((img[0::2, 0::2] + img[0::2, 1::2]) + (img[1::2, 0::2] + img[1::2, 1::2])) * F(0.25)
    out[..., 3] = 1.0
    return out


def resolve(img, samples):
    for _ in range({1: 0, 2: 1, 4: 2}[samples]):
        img = resolve2(img)
    return img


def quantise(img):
    """(uint8)(min(max(c, 0), 1) * 255.0f + 0.5f), NaN -> 0; alpha 255."""
    c = np.asarray(img, dtype=F)[..., :3]
    with np.errstate(all="ignore"):
        t = np.where(c > 0, c, F(0))  # (a NaN compares false: 0)
        t = np.where(t < 1, t, F(1))
        q = (t * F(255.0) + F(0.5)).astype(np.uint32).astype(np.uint8)
    out = np.empty(c.shape[:-1] + (4,), dtype=np.uint8)
    out[..., :3] = q
    out[..., 3] = 255
    return out


def oracle_forward(rows, W, H, exact_exp=False):
    """The reference's forward loop over `rows` at W x H."""
    L = O.lib()
    rows = np.ascontiguousarray(rows, dtype=O.SPLAT_DTYPE)
    img = np.zeros((H, W, 4), dtype=F)
    L.s2do_set_exact_exp(1 if exact_exp else 0)
    try:
        L.s2do_forward_rows(O._p(rows), len(rows), W, H, 0, H, O._p(img), None)
    finally:
        L.s2do_set_exact_exp(0)
    return img


# ---- refusals: (what differs from a good configuration, refused?) ---------------------------------------------------------
GOOD = dict(out_width=53, out_height=37, origin_x=5.25, origin_y=3.5, zoom=2.5, filter_var=0.0, samples=1, format=0)
INF, NAN = float("inf"), float("nan")
REFUSAL_TABLE = [
    ({}, False),
    ({"samples": 0}, False), ({"samples": 2}, False), ({"samples": 4}, False), ({"format": 1}, False),
    ({"filter_var": 0.75}, False), ({"origin_x": -1e6, "origin_y": 1e6}, False), ({"zoom": 1e-3}, False),
    ({"out_width": 65536, "out_height": 1}, False), ({"out_width": 16384, "out_height": 16384, "samples": 4}, False),
    ({"struct_size_delta": 4}, True), ({"struct_size_delta": -4}, True),
    ({"out_width": 0}, True), ({"out_height": 0}, True), ({"out_width": -3}, True),
    ({"out_width": 65537}, True), ({"out_height": 65537}, True),
    ({"out_width": 32769, "samples": 2}, True), ({"out_height": 16385, "samples": 4}, True),
    ({"zoom": 0.0}, True), ({"zoom": -1.0}, True), ({"zoom": INF}, True), ({"zoom": NAN}, True),
    ({"origin_x": INF}, True), ({"origin_y": NAN}, True), ({"origin_x": -INF}, True),
    ({"filter_var": -0.5}, True), ({"filter_var": INF}, True), ({"filter_var": NAN}, True),
    ({"samples": 3}, True), ({"samples": -1}, True), ({"samples": 8}, True),
    ({"format": 2}, True), ({"format": 0xFFFFFFFF}, True),
]


def make_config(struct_type, **changes):
    """A ctypes s2d_view_config: GOOD with `changes` applied."""
    fields = dict(GOOD)
    delta = changes.pop("struct_size_delta", 0)
    fields.update(changes)
    cfg = struct_type()
    cfg.struct_size = C.sizeof(struct_type) + delta
    for k, v in fields.items():
        setattr(cfg, k, v)
    return cfg
