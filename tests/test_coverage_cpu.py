"""CPU tests of the coverage channel (S2D_CFG_COVERAGE): the flag in the header and the binding, what
s2d_create and s2d_multi_create refuse before any device work, the formula of the backward walk as a derivative, and the RGBA
side of the host program's image files.

The formula: coverage is A = sum_i T_i alpha_i, the reference's colour sum (main.cpp:529-531) for a channel whose colour is 1,
so its derivative with respect to alpha_i is main.cpp:627-628 with c = 1: T_i - S_a / (1 - alpha_i), S_a = A - A_running.
tests/coverage_ref.py restates the blend and that expression in float64 with the exact exponential; here central differences
of sum w * A in every geometric parameter and the opacity are held to it, with the tolerance tests/test_derivation_fd.py uses for
the colour channels.  That shows the formula is the derivative; tests/test_gpu_coverage.py shows the kernel is the formula.
"""
import ctypes as C
import importlib
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import coverage_ref as CR
import oracle_lib as O

S2D = importlib.import_module("2dgaussiansplatting_amd")
HEADER = os.path.join(O.ROOT, "include", "splat2d.h")
HC_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostcheck")


@pytest.fixture(scope="module")
def lib():
    S2D._build.build_hip_library()
    return S2D.load_library()


def _config(flags, W=64, H=64, row_begin=0, row_end=0):
    cfg = S2D._Config()
    cfg.struct_size = C.sizeof(S2D._Config)
    cfg.width, cfg.height, cfg.n_splats = W, H, 10
    cfg.row_begin, cfg.row_end = row_begin, row_end
    cfg.flags = flags
    return cfg


def test_the_header_defines_the_flag_and_the_binding_exports_it():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"^[ \t]*#[ \t]*define[ \t]+S2D_CFG_COVERAGE[ \t]+(0[xX][0-9a-fA-F]+)[uU]?[ \t]*$", src, flags=re.M)
    assert m and int(m.group(1), 0) == 0x80
    assert S2D.S2D_CFG_COVERAGE == 0x80
    import inspect
    p = inspect.signature(S2D.Trainer.__init__).parameters
    assert list(p)[-1] == "coverage" and p["coverage"].default is False


@pytest.mark.parametrize("other", ["S2D_CFG_COUNT_PAIRS", "S2D_CFG_EXACT_EXP", "S2D_CFG_REFERENCE_ORDER"])
def test_create_refuses_the_flag_with_the_modes_that_have_no_coverage_kernels(lib, other):
    h = C.c_void_p()
    cfg = _config(S2D.S2D_CFG_COVERAGE | getattr(S2D, other))
    assert lib.s2d_create(C.byref(cfg), C.byref(h)) == 1 and not h.value


@pytest.mark.parametrize("rows", [(0, 32), (16, 64), (16, 48)])
def test_create_refuses_the_flag_with_a_row_slab(lib, rows):
    h = C.c_void_p()
    cfg = _config(S2D.S2D_CFG_COVERAGE, row_begin=rows[0], row_end=rows[1])
    assert lib.s2d_create(C.byref(cfg), C.byref(h)) == 1 and not h.value


def test_multi_create_refuses_the_flag(lib):
    h = C.c_void_p()
    devs = (C.c_int32 * 2)(0, 1)
    cfg = _config(S2D.S2D_CFG_COVERAGE)
    assert lib.s2d_multi_create(C.byref(cfg), devs, 1, 0, C.byref(h)) == 1 and not h.value
    assert lib.s2d_multi_create(C.byref(cfg), devs, 2, 0, C.byref(h)) == 1 and not h.value


# ---------------------------------------------------------------------------------------------------------
# the formula is the derivative
# ---------------------------------------------------------------------------------------------------------
def fd_scene():
    """12 x 12, 6 splats that overlap each other and the image, no alpha near 1."""
    rng = np.random.default_rng(612)
    n, W, H = 6, 12, 12
    s = np.zeros((n, 9))
    s[:, 0] = rng.uniform(2, 10, n)
    s[:, 1] = rng.uniform(2, 10, n)
    s[:, 2:4] = rng.uniform(1.5, 4.0, (n, 2))
    s[:, 4] = rng.uniform(-3, 3, n)
    s[:, 5:8] = rng.uniform(0, 1, (n, 3))
    s[:, 8] = rng.uniform(0.2, 0.85, n)
    y, x = np.mgrid[0:H, 0:W]
    w = np.sin(0.9 * x + 0.4 * y) + 0.3  # signed, spatially varying
    return s, W, H, w


def test_coverage_telescopes_to_one_minus_the_throughput():
    s, W, H, _ = fd_scene()
    al = CR.alphas_of(s, W, H)
    assert np.allclose(CR.coverage_of(s, W, H), 1.0 - np.prod(1.0 - al, axis=0), rtol=0, atol=1e-14)


@pytest.mark.parametrize("i", range(6))
def test_the_alpha_term_of_the_backward_walk_is_the_derivative_of_the_coverage(i):
    s, W, H, w = fd_scene()
    g = CR.coverage_grads(s, W, H, w)
    assert not g[:, 5:8].any() and np.abs(g[:, [0, 1, 2, 3, 4, 8]]).min() > 0
    loss = lambda s9: float(np.sum(w * CR.coverage_of(s9, W, H)))
    h = 1e-6
    for k in (0, 1, 2, 3, 4, 8):
        sp, sm = s.copy(), s.copy()
        sp[i, k] += h
        sm[i, k] -= h
        fd = (loss(sp) - loss(sm)) / (2 * h)
        assert fd == pytest.approx(g[i, k], rel=1e-6, abs=1e-10), (i, k)   # tests/test_derivation_fd.py, the colour channels
    for k in (5, 6, 7):  # a colour does not reach the coverage
        sp = s.copy()
        sp[i, k] += 0.1
        assert loss(sp) == loss(s)


# ---------------------------------------------------------------------------------------------------------
# the references of tests/test_gpu_coverage_limits.py, on their own
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opacity", [False, True], ids=["fixed_opacity", "optimize_opacity"])
@pytest.mark.parametrize("name", CR.SCENES)
def test_the_four_channel_loop_is_ten_times_closer_to_itself_than_the_bar_it_is_used_with(name, opacity):
    """coverage_ref.FourChannelOracle adds the gradients of two oracle passes.  Whether the two fp32 results are added ("f32")
    or all terms are summed in double and rounded once ("f64") is a choice the GPU does not share with either: after five
    iterations the two must agree ten times better than the bar the GPU is held to against "f32" (the update bar of
    tests/test_gpu_parity.py::test_training_steps_random_sweep).  Measured: mini 1.3e-4 of 2.9e-3 (opacity on), 17 x 17 1.9e-6
    of 4.1e-4, stack 1.9e-6 of 1.1e-3."""
    mse32, sp32 = CR.five_steps(name, opacity, "f32")
    mse64, sp64 = CR.five_steps(name, opacity, "f64")
    bar = CR.update_bar(sp32)
    worst = float(np.abs(sp32 - sp64).max())
    print("\n[coverage] %s opacity=%s: max |f32 - f64| after 5 steps %.3e, bar %.3e" % (name, opacity, worst, bar))
    assert np.isfinite(sp32).all() and np.isfinite(mse32).all() and mse32[0] == mse64[0]
    assert worst <= 0.1 * bar, (worst, bar)
    np.testing.assert_allclose(mse64, mse32, rtol=2e-6)   # (a tenth of the trace bar)
    s0 = CR.scene(name)[1]
    moved = np.abs(sp32 - s0)
    assert moved[:, CR.GEOM[:5]].max() > 10 * bar / 5 and (moved[:, 8].any() if opacity else not moved[:, 8].any())
    # ... and the fourth channel is at work: the plain oracle alone ends somewhere else
    o = CR.oracle_of(CR.scene(name)[0], s0)
    o.optimize_opacity = opacity
    for _ in range(5):
        o.step()
    assert np.abs(o.splats.view(np.float32).reshape(-1, 9) - sp32).max() > bar


def test_the_sweep_is_not_trivial():
    """Over seeds 0 .. 23 of coverage_ref.sweep_case the oracle twin's coverage has pixels at exactly 0, in (0.05, 0.95) and
    above 0.99, every splat count and every variant occurs with splats, and the twin's gradient under a signed upstream is
    finite for every seed (a seed whose oracle gradient is not would be replaced, not forgiven)."""
    import test_image_grads_cpu as IG
    zero = mid = high = 0
    counts, with_splats = set(), set()
    for seed in CR.SWEEP_SEEDS:
        W, H, n, s, tgt = CR.sweep_case(seed)
        assert tgt.shape == (H, W, 4) and len(s) == n and 1 <= W < 300 and 1 <= H < 220
        assert W * H == 1 or len(np.unique(tgt[..., 3])) > 1
        counts.add(n)
        if n == 0:
            continue
        with_splats.add(seed % 4)
        o = CR.oracle_of(tgt, CR.white_twin(s))
        frame = o.forward().copy()
        cov = frame[..., 0]
        zero, mid, high = zero + int((cov == 0).sum()), mid + int(((cov > 0.05) & (cov < 0.95)).sum()), high + int((cov > 0.99).sum())
        gu = np.zeros(frame.shape, dtype=np.float32)
        gu[..., 0] = CR.signed_upstream(H, W, seed)
        o.ref = np.ascontiguousarray(IG.pseudo_target(frame, gu))
        d, dsum, dabs = o.backward_stats()
        assert np.isfinite(d.view(np.float32)).all() and np.isfinite(dsum).all() and np.isfinite(dabs).all(), seed
    print("\n[coverage] sweep: %d pixels at 0, %d in (0.05, 0.95), %d above 0.99; counts %s" % (zero, mid, high, sorted(counts)))
    assert zero > 1000 and mid > 1000 and high > 1000
    assert counts == {0, 1, 3, 40, 300, 700} and with_splats == {0, 1, 2, 3}


# ---------------------------------------------------------------------------------------------------------
# RGBA files of the host program
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def io_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("image_io") / "s2d_image_io_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(HC_DIR, "s2d_image_io_main.cpp"), "-lz"])
    return exe


def _rgba(W=23, H=9, seed=3):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    a[0, :4, 3] = 0      # transparent, with colour left behind it
    a[1, :4, 3] = 255
    return a


def _read(io_exe, path, out):
    subprocess.check_call([io_exe, "read", str(path), str(out)])
    d = open(out, "rb").read()
    w, h = struct.unpack("<ii", d[:8])
    return np.frombuffer(d[8:], dtype=np.uint8).reshape(h, w, 4)


def test_png_rgba_written_and_read_back_gives_the_same_bytes(io_exe, tmp_path):
    a = _rgba()
    open(tmp_path / "in.rgba", "wb").write(a.tobytes())
    subprocess.check_call([io_exe, "write", str(a.shape[1]), str(a.shape[0]), str(tmp_path / "in.rgba"), str(tmp_path / "a.png")])
    assert _read(io_exe, tmp_path / "a.png", tmp_path / "back.bin").tobytes() == a.tobytes()
    from PIL import Image
    im = Image.open(tmp_path / "a.png")                      # our RGBA PNG is a valid PNG
    assert im.mode == "RGBA" and np.array_equal(np.asarray(im), a)


def test_files_without_alpha_read_as_opaque(io_exe, tmp_path):
    from PIL import Image
    a = _rgba()
    Image.fromarray(a[..., :3].copy()).save(tmp_path / "rgb.png")
    got = _read(io_exe, tmp_path / "rgb.png", tmp_path / "rgb.bin")
    assert np.array_equal(got[..., :3], a[..., :3]) and (got[..., 3] == 255).all()
    Image.fromarray(a[..., 0].copy()).save(tmp_path / "grey.png")
    got = _read(io_exe, tmp_path / "grey.png", tmp_path / "grey.bin")
    assert np.array_equal(got[..., 1], a[..., 0]) and (got[..., 3] == 255).all()
    Image.fromarray(a[..., [0, 3]].copy(), "LA").save(tmp_path / "la.png")   # grey with alpha keeps it
    got = _read(io_exe, tmp_path / "la.png", tmp_path / "la.bin")
    assert np.array_equal(got[..., 2], a[..., 0]) and np.array_equal(got[..., 3], a[..., 3])
    Image.fromarray(a).save(tmp_path / "pil.png")                             # a PNG with filters and alpha, written by PIL
    assert np.array_equal(_read(io_exe, tmp_path / "pil.png", tmp_path / "pil.bin"), a)
    mini = os.path.join(O.GOLDEN, "squirrel_cls_mini_268x213.s2di")
    got = _read(io_exe, mini, tmp_path / "mini.bin")
    assert np.array_equal(got[..., :3], O.load_s2di(mini)) and (got[..., 3] == 255).all()


def test_the_coverage_target_is_premultiplied_and_the_output_is_straight(io_exe, tmp_path):
    from PIL import Image
    a = _rgba()
    Image.fromarray(a).save(tmp_path / "t.png")
    subprocess.check_call([io_exe, "target", str(tmp_path / "t.png"), str(tmp_path / "t.bin")])
    d = open(tmp_path / "t.bin", "rb").read()
    t = np.frombuffer(d[8:], dtype=np.float32).reshape(a.shape)
    al = a[..., 3].astype(np.float32) / np.float32(255.0)
    want = np.empty(a.shape, dtype=np.float32)
    want[..., :3] = (a[..., :3].astype(np.float32) / np.float32(255.0)) * al[..., None]
    want[..., 3] = al
    assert t.tobytes() == want.tobytes()
    # ... and back: rgb / A where A > 0, otherwise 0 -- the file's bytes wherever alpha leaves the colour enough precision
    open(tmp_path / "t.f32", "wb").write(t.tobytes())
    subprocess.check_call([io_exe, "straight", str(a.shape[1]), str(a.shape[0]), str(tmp_path / "t.f32"), str(tmp_path / "s.bin")])
    s = np.frombuffer(open(tmp_path / "s.bin", "rb").read(), dtype=np.uint8).reshape(a.shape)
    assert np.array_equal(s[..., 3], a[..., 3])
    assert not s[a[..., 3] == 0].any()
    assert np.array_equal(s[a[..., 3] > 0][:, :3], a[a[..., 3] > 0][:, :3])


def test_straight_rgba8_is_quantise_straight(io_exe, tmp_path):
    """coverage_ref.straight_rgba8, which the GPU tests of the host program compare files with, against the C++ it restates:
    a random float image with a = 0, a < 0, a tiny (the quotient overflows), rgb > a, negative colours and exact byte steps."""
    rng = np.random.default_rng(11)
    W, H = 37, 21
    f = np.zeros((H, W, 4), dtype=np.float32)
    f[..., 3] = rng.uniform(0.0, 1.0, (H, W))
    f[..., :3] = rng.uniform(0.0, 1.0, (H, W, 3)) * f[..., 3:4]            # premultiplied, as image0 is
    f[0, :, 3] = 0.0                                                       # transparent, with colour left behind it
    f[0, :, :3] = rng.uniform(-1, 1, (W, 3))
    f[1, :, 3] = -rng.uniform(0, 1, W)
    f[2, :, 3] = np.array([1e-45, 1e-38, 1e-30, 1e-12], dtype=np.float32)[np.arange(W) % 4]   # c / a overflows or is huge
    f[3, :, :3] = f[3, :, 3:4] * rng.uniform(1.0, 3.0, (W, 3))             # rgb > a
    f[4, :, :3] = -f[4, :, :3]
    f[5, :, 3] = 1.0 + rng.uniform(0, 1, W)                                # coverage above 1 clamps
    k = np.arange(W, dtype=np.float32)
    f[6, :, 3] = 1.0
    f[6, :, 0] = (k + np.float32(0.5)) / np.float32(255.0)                 # on the rounding boundary of a byte
    f[6, :, 1] = k / np.float32(255.0)
    f[7, :, 3] = (k * 7 % 256) / np.float32(255.0)
    assert np.isfinite(f).all()
    open(tmp_path / "f.f32", "wb").write(f.tobytes())
    subprocess.check_call([io_exe, "straight", str(W), str(H), str(tmp_path / "f.f32"), str(tmp_path / "s.bin")])
    want = np.frombuffer(open(tmp_path / "s.bin", "rb").read(), dtype=np.uint8).reshape(H, W, 4)
    got = CR.straight_rgba8(f)
    assert got.dtype == np.uint8 and got.tobytes() == want.tobytes()
    assert not got[0].any() and not got[1].any() and (got[2, :, 3] == 0).all() and (got[2, :, :3] == 255).any()
    assert (got[3, :, :3] == 255).all() and not got[4, :, :3].any() and (got[5, :, 3] == 255).all()
    assert len(np.unique(got[..., 3])) > 200 and len(np.unique(got[..., :3])) > 200


def test_the_host_program_refuses_coverage_with_what_it_cannot_combine(tmp_path):
    S2D._build.build_hip_library()
    exe = S2D._build.build_host_program()
    base = [exe, "--synthetic", "64x64", "--splats", "16", "--iters", "1", "--coverage"]
    for extra in (["--gpus", "2"], ["--loss-weights", "0,0.8,0.2"], ["--relocate-every", "10"], ["--reseed-every", "10"],
                  ["--prune-every", "10"], ["--reference-order"], ["--out-image", str(tmp_path / "x.ppm")]):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        assert r.returncode == 2 and "--coverage" in r.stderr, (extra, r.stderr)
