"""Tile lists and raster at the geometry limits s2d_create accepts (images of up to 65536 x 65536), from the tall side and
the many-tiles side: the code is written around these limits and the rest of the suite stays far below them.

  * more than 1024 tile rows: tl_chunk_table_kernel cuts the rows over its 1024 threads by more than one each; the row sort
    of the two-level builder has 11 and 12 key bits under the 18 bits of column range it must carry along; at H = 65536 a row
    key uses bit 11, a rectangle has ty1 = 4095, and the synthetic target is launched with 65536 grid rows;
  * exactly 512 tile columns (8192 px) with rectangles tx0 = 0 .. tx1 = 511: the full nine bits of a row entry's column
    range and all 512 columns of the column pass in LDS;
  * 4096 tile columns (65536 px): the generic builder at the uint16_t edge of TileRect;
  * more than 65536 tiles through the generic builder: 17 key bits, three radix passes, the list-boundary variant as a
    one-bit last pass;
  * slabs with a large first tile row, halo masks for 32 ranks (bit 31);
  * iteration numbers across the 65536 slots of the squared-error ring.

Bars: those of test_gpu_parity.py (module docstring), in the form test_images_wider_than_512_tile_columns states them for
strips on which the oracle's own sequential fp32 sum drifts: framebuffer bit-exact, (a) the GPU's sums within
max(1e-6, b_ref / 10) of the exact sum and (b) no further from it than the oracle's (b_ref), (c) within max(1e-4, 10 b_ref)
of the oracle's fp32 value.  Everything else here is compared on bytes.  The oracle's part of every scene is computed once
(functools.lru_cache) and shared by the tests; nothing writes to it afterwards.
"""
import functools
import importlib

import numpy as np
import pytest

import oracle_lib as O
from oracle_lib import random_splats
from test_gpu_parity import REL, _lists
from test_gpu_reference_order import same32, same64

pytestmark = pytest.mark.gpu

S2D = importlib.import_module("2dgaussiansplatting_amd")

# name: (W, H, n, seed)
SCENES = {
    "1025_tile_rows": (40, 16400, 3000, 41),      # per = 2 in tl_chunk_table_kernel, 11 row bits
    "4096_tile_rows": (24, 65536, 6000, 42),      # the height limit: per = 4, row bit 11, ty1 = 4095, 65536 grid rows
    "4096_tile_columns": (65536, 24, 6000, 43),   # the width limit: generic builder, tx1 = 4095
    "512_tile_columns": (8192, 48, 4000, 44),     # the two-level builder's limit, plus four splats over all 512 columns
}
TWO_LEVEL = [k for k, v in SCENES.items() if (v[0] + 15) // 16 <= 512]


def scene_splats(name):
    W, H, n, seed = SCENES[name]
    s = random_splats(n, W, H, seed)
    if name == "512_tile_columns":
        # Four splats of sx = 4096 (outside Adam's clamp; s2d_set_splats takes what it is given and the oracle renders it)
        # centred, at both ends and off-centre: 3 sx is more than the image is wide, so each one's rectangle is tx0 = 0 ..
        # tx1 = 511 wherever it sits.  In front of the others, so that they are alive in every pixel and share the first
        # chunk of every tile row they cover: 4 x 512 pairs, more than the 1536 the chunk's staging buffer holds.
        wide = np.zeros(4, dtype=O.SPLAT_DTYPE)
        wide["pos"] = [(4096.0, 24.0), (0.0, 5.0), (8191.0, 40.0), (2500.0, 30.0)]
        wide["sx"] = 4096.0
        wide["sy"] = [8.0, 3.0, 20.0, 1.5]
        wide["rot"] = 0.0
        wide["color"] = [(0.9, 0.2, 0.1), (0.1, 0.8, 0.3), (0.2, 0.3, 0.9), (0.7, 0.7, 0.1)]
        wide["opacity"] = 0.05
        s = np.concatenate([wide, s])
    return s


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> dict: geometry, splats, synthetic target, and the oracle's framebuffer, fp32 gradients, exact sums and term
    magnitudes.  Read-only from here on."""
    W, H, _, _ = SCENES[name]
    s = scene_splats(name)
    tgt = O.synthetic_target(W, H)
    o = O.OracleTrainer(tgt, len(s))
    o.splats[:] = s
    image = o.forward().copy()
    w32, dsum, dabs = o.backward_stats()
    r = dict(W=W, H=H, n=len(s), splats=s, target=tgt, image=image, mse=o.mse(),
             w32=w32.view(np.float32).reshape(-1, 9).astype(np.float64), dsum=dsum, dabs=dabs)
    assert (dabs > 0).any(axis=1).all()   # every splat reaches a live pixel: no gradient is compared with nothing
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def oracle_three_steps(name):
    sc = scene(name)
    o = O.OracleTrainer(sc["target"], sc["n"])
    o.splats[:] = sc["splats"]
    return tuple(o.step()[1] for _ in range(3))


def loaded(sc, **kw):
    t = S2D.Trainer(sc["W"], sc["H"], sc["n"], **kw)
    t.set_target(sc["target"])
    t.set_splats(sc["splats"])
    return t


def scaled_bars(name, got, sc):
    """The three gradient bars relative to the oracle's own distance from the exact sum; prints and returns (a, b_ref, c)."""
    gg = got.view(np.float32).reshape(-1, 9).astype(np.float64)
    ww, dsum, dabs = sc["w32"], sc["dsum"], sc["dabs"]
    nz = dabs > 0
    assert np.all(gg[~nz] == 0)
    b_ref = float((np.abs(ww - dsum)[nz] / dabs[nz]).max())
    a = float((np.abs(gg - dsum)[nz] / dabs[nz]).max())
    c = float((np.abs(gg - ww)[nz] / np.maximum(np.abs(ww[nz]), 0.02 * dabs[nz])).max())
    print("%s: a %.3g  b_ref %.3g  c %.3g" % (name, a, b_ref, c))
    assert a <= max(1e-6, 0.1 * b_ref) and a <= b_ref, (a, b_ref)
    assert c <= max(REL, 10.0 * b_ref), (c, b_ref)
    return a, b_ref, c


# ---------------------------------------------------------------------------------------------
# the four scenes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SCENES))
def test_forward_and_gradients(name):
    """Default flags: framebuffer bit-exact, gradients within the three bars (every pixel, every scalar)."""
    sc = scene(name)
    with loaded(sc) as t:
        t.forward()
        assert t.get_image().tobytes() == sc["image"].tobytes()
        t.backward()   # (the backward pass is what sums the squared error: s2d_get_mse is a state error before it)
        assert abs(t.mse() - sc["mse"]) <= 1e-9 * sc["mse"]
        g = t.get_grads()
        assert t.stats()["pairs_binned"] > sc["n"]
    # b_ref as the CPU oracle gives it: 1.06e-5, 3.12e-5, 8.65e-6, 9.43e-5 (the four 8192-px splats of the last scene sum
    # 390 000 terms per scalar).  Measured on an MI355X, in the order of SCENES (float atomics: the last digits vary from
    # run to run): a 5.9e-7, 1.2e-6, 7.5e-7, 5.5e-7 against bars of 1.1e-6, 3.1e-6, 1e-6, 9.4e-6;
    # c 5.6e-5, 6.0e-5, 4.6e-5, 1.7e-4 against bars of 1.1e-4, 3.1e-4, 1e-4, 9.4e-4.
    scaled_bars(name, g, sc)


@pytest.mark.parametrize("name", TWO_LEVEL)
def test_both_builders_give_the_same_lists(name):
    """Wherever the two-level builder applies (up to 512 tile columns): offsets and lists word for word those of the
    generic builder, and the same framebuffer -- the oracle's."""
    sc = scene(name)
    a = _lists(sc["W"], sc["H"], sc["n"], sc["splats"], False)
    b = _lists(sc["W"], sc["H"], sc["n"], sc["splats"], True)
    assert (a[0], a[1]) == (b[0], b[1]) == ((sc["W"] + 15) // 16, (sc["H"] + 15) // 16)
    assert np.array_equal(a[2], b[2]), "tile offsets differ"
    assert np.array_equal(a[3], b[3]), "tile lists differ"
    assert len(a[3]) > sc["n"]
    assert a[4].tobytes() == b[4].tobytes() == sc["image"].tobytes()
    if name == "512_tile_columns":
        # the four wide splats head the list of every tile: their rectangles are tx0 = 0 .. tx1 = 511 over all three rows
        off = a[2].astype(np.int64)
        assert np.all(np.diff(off) >= 4)
        assert np.array_equal(a[3][off[:-1, None] + np.arange(4)], np.tile(np.arange(4, dtype=np.uint32), (len(off) - 1, 1)))


@pytest.mark.parametrize("name", list(SCENES))
def test_deterministic_gradients(name):
    """deterministic=True: the same bits from two contexts, and the same bars."""
    sc = scene(name)
    res = []
    for _ in range(2):
        with loaded(sc, deterministic=True) as t:
            t.forward()
            t.backward()
            res.append(t.get_grads())
    assert res[0].tobytes() == res[1].tobytes()
    # measured on an MI355X, same bars as above: a 6.2e-7, 7.4e-7, 4.7e-7, 1.05e-6; c 5.6e-5, 5.9e-5, 4.7e-5, 1.7e-4
    scaled_bars(name + " deterministic", res[0], sc)


@pytest.mark.parametrize("name", list(SCENES))
def test_three_training_steps(name):
    """s2d_step against three oracle steps: the first MSE to 1e-9 (same framebuffer), the others to the 1e-4 of
    test_images_wider_than_512_tile_columns, for the reason given there (one-pixel-thin and 1024-px splats side by side:
    a last-place difference in a gradient sum flips a pixel's inclusion a step later)."""
    sc = scene(name)
    want = oracle_three_steps(name)
    with loaded(sc) as t:
        got = t.step(3)
    print("%s: mse" % name, list(got), "oracle", list(want))
    # measured on an MI355X: the second value within 1e-9 .. 8e-8 of the oracle's, the third within 7e-7 .. 1.3e-5
    assert abs(got[0] - want[0]) <= 1e-9 * want[0]
    np.testing.assert_allclose(got, want, rtol=1e-4)


@pytest.mark.parametrize("name", list(SCENES))
def test_synthetic_target_on_the_device(name):
    """s2d_set_target_synthetic (one grid row per image row: 65536 of them at the height limit) leaves the target that
    oracle_lib.synthetic_target uploads: same framebuffer, same MSE bytes, and -- deterministic sums, which read every
    pixel's image0 - imageRef -- the same gradient bytes."""
    sc = scene(name)
    res = []
    for synthetic in (False, True):
        with S2D.Trainer(sc["W"], sc["H"], sc["n"], deterministic=True) as t:
            if synthetic:
                t.set_target_synthetic()
            else:
                t.set_target(sc["target"])
            t.set_splats(sc["splats"])
            t.forward()
            img = t.get_image()
            t.backward()
            res.append((img.tobytes(), np.float64(t.mse()).tobytes(), t.get_grads().tobytes()))
    assert res[0][0] == res[1][0] == sc["image"].tobytes()
    assert res[0][1] == res[1][1], "MSE against the device's synthetic target differs"
    assert res[0][2] == res[1][2], "gradients against the device's synthetic target differ"


# ---------------------------------------------------------------------------------------------
# reference order, slabs and halo masks in a tall image
# ---------------------------------------------------------------------------------------------
def test_reference_order_at_height():
    """S2D_CFG_REFERENCE_ORDER on 1025 tile rows (400 splats keep the per-pair scratch small): framebuffer, gradients, MSE
    and the state after Adam are the oracle's bytes, as in test_gpu_reference_order.py::test_adversarial_scenes."""
    W, H, n = 40, 16400, 400
    tgt = O.synthetic_target(W, H)
    o = O.OracleTrainer(tgt, n)
    o.splats[:] = random_splats(n, W, H, 45)
    img = o.forward().copy()
    d = o.backward().copy()
    mse = o.mse()
    assert np.isfinite(d.view(np.float32)).all() and (d.view(np.float32).reshape(n, 9) != 0).any(axis=1).all()
    with S2D.Trainer(W, H, n, reference_order=True) as t:
        t.set_target(tgt)
        t.set_splats(o.splats.view(S2D.SPLAT_DTYPE))
        t.forward()
        t.backward()
        assert same32(t.get_image(), img)
        assert same32(t.get_grads(), d)
        assert same64(t.mse(), mse)
        t.adam_step()
        assert o.adam() == 0
        assert same32(t.get_splats(), o.splats)
        adams, b1, b2, _ = t.get_adam()
        assert same32(adams, o.adams)
        assert same32(np.float32(b1), o.beta1t[0]) and same32(np.float32(b2), o.beta2t[0])


@pytest.mark.parametrize("r0,r1", [(32768, 32816), (65488, 65536), (0, 16)])
def test_slabs_deep_in_a_tall_image(r0, r1):
    """Slab contexts of the 24 x 65536 scene whose first tile row is 2048, 4093 and 0: the slab's rows bit-exact against
    the oracle's, gradients of those rows within the usual bars (O.grad_bars: a few hundred terms per scalar, the oracle's
    sum does not drift here)."""
    sc = scene("4096_tile_rows")
    o = O.OracleTrainer(sc["target"], sc["n"])
    o.splats[:] = sc["splats"]
    want = o.forward(r0, r1)[r0:r1].copy()
    assert want.tobytes() == sc["image"][r0:r1].tobytes()
    w32, dsum, dabs = o.backward_stats(r0, r1)
    assert (dabs > 0).any()
    with loaded(sc, row_begin=r0, row_end=r1) as t:
        t.forward()
        assert t.get_image_rows().tobytes() == want.tobytes()
        t.backward()
        g = t.get_grads()
        assert 0 < t.stats()["pairs_binned"] < sc["n"] * 8
    # measured on an MI355X: a 1.5e-7, 1.1e-7, 6.6e-8 (b_ref 1.2e-6, 1.4e-6, 3.6e-7); c 7.2e-6, 3.5e-6, 2.7e-6
    m = O.grad_bars(g.view(np.float32), w32.view(np.float32), dsum, dabs, REL)
    print("rows %d..%d: a %.3g  b_ref %.3g  c %.3g" % (r0, r1, m["a_gpu_vs_exact"], m["b_ref_vs_exact"], m["c_gpu_vs_oracle"]))


def test_halo_masks_of_32_slabs():
    """s2d_halo_masks for 32 equal slabs of 2048 rows against the formula of test_row_level_abi_calls_against_numpy; rank 31
    is bit 31 of the mask, so the comparison is on uint32."""
    D = importlib.import_module("2dgaussiansplatting_amd.distributed")
    sc = scene("4096_tile_rows")
    world, margin = 32, 2.0
    bounds = [2048 * q for q in range(world + 1)]
    with loaded(sc) as t:
        m = D.HipHaloOps(t, sc["n"], "cuda").halo_masks(bounds, margin).cpu().numpy().view(np.uint32)
    sp = sc["splats"].view(np.float32).reshape(-1, 9)
    reach = np.float32(3.0) * np.maximum(sp[:, 2], sp[:, 3]) + np.float32(2.0) + np.float32(margin)
    want = np.zeros(sc["n"], dtype=np.uint32)
    for q in range(world):
        want |= ((sp[:, 1] + reach >= np.float32(bounds[q])) & (sp[:, 1] - reach <= np.float32(bounds[q + 1]))).astype(np.uint32) << np.uint32(q)
    assert np.array_equal(m, want) and (m != 0).all()
    assert (m >> np.uint32(31)).any() and (m & np.uint32(1)).any() and len(np.unique(m)) > 32


# ---------------------------------------------------------------------------------------------
# more than 65536 tiles through the generic builder
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("long_lists", [False, True], ids=["init", "long_lists"])
def test_generic_builder_with_three_radix_passes(long_lists):
    """4112 x 4112: 257 x 257 = 66049 tiles, 17 key bits -- three radix passes, the last of one bit and in the variant that
    records list boundaries instead of keys -- on init() with 100 000 splats, and the same with 20 splats grown to
    sx = sy = 1024 (lists of up to 20 more entries in every tile, 1.3 M pairs more).  Offsets, lists and the whole
    framebuffer (2 x 270 MB) equal the two-level builder's, word for word."""
    W, H, n = 4112, 4112, 100_000
    with S2D.Trainer(W, H, n) as t:
        t.init()
        sp = t.get_splats()
    if long_lists:
        sp["sx"][::5000] = 1024.0
        sp["sy"][::5000] = 1024.0
    a = _lists(W, H, n, sp, False)
    b = _lists(W, H, n, sp, True)
    assert (a[0], a[1]) == (b[0], b[1]) == (257, 257)
    assert np.array_equal(a[2], b[2]), "tile offsets differ"
    assert np.array_equal(a[3], b[3]), "tile lists differ"
    assert len(a[3]) > (1_000_000 if long_lists else n)
    assert a[2][-1] == len(a[3]) and (np.diff(a[2].astype(np.int64)) > 0).any()
    assert np.array_equal(a[4], b[4])


# ---------------------------------------------------------------------------------------------
# the squared-error ring
# ---------------------------------------------------------------------------------------------
def test_iteration_numbers_across_the_sqerr_ring():
    """The squared errors of the last 65536 iterations live in a ring indexed by iteration % 65536.  Two deterministic
    contexts from the same splats, moments and beta powers, one counting from 0 and one from 65530, run 12 iterations:
    the second one's slots wrap, and nothing else may differ."""
    W, H, n = 96, 80, 300
    tgt = O.synthetic_target(W, H)
    s = random_splats(n, W, H, 3)
    res = []
    for first in (0, 65530):
        with S2D.Trainer(W, H, n, deterministic=True) as t:
            t.set_target(tgt)
            t.set_splats(s)
            adams, b1, b2, _ = t.get_adam()
            t.set_adam(adams, b1, b2, first)
            mse = t.step(12)
            ad, c1, c2, it = t.get_adam()
            assert it == first + 12 == t.stats()["iterations"]
            res.append((mse.tobytes(), t.get_splats().tobytes(), ad.tobytes(), (c1, c2), t.sqerr_trace(first, 12)))
    assert res[1][4].tobytes() == res[0][4].tobytes()
    assert np.isfinite(res[0][4]).all() and len(set(res[0][4])) == 12
    for k, what in enumerate(["MSEs", "splats", "moments", "beta powers"]):
        assert res[0][k] == res[1][k], what
