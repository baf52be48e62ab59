"""CPU tests of the backdrop (include/splat2d_backdrop.h): the oracle helper of tests/backdrop_ref.py pinned
on its own, the backward walk's expression as the derivative of the composite, and the surface -- the five exported symbols, the
header as C, the binding's table against the header, the kernels the new unit emits, the refusals that need no device and the
argument errors of `splat2d_train --background`.  No GPU.

The derivative: I = sum_i c_i T_i alpha_i + T_final * B.  The backward walk reads the final colour from image0 and forms
S = fin - running (main.cpp:627); with I stored in image0, S carries T_final * B, and c_i T_i - S / (1 - alpha_i) (main.cpp:628) is
dI/d alpha_i.  tests/backdrop_ref.py restates the composite and that expression in float64 with the exact exponential and no
cut-off; central differences of sum w * I in every parameter are held to it with the scheme and the bar of
tests/test_coverage_cpu.py.  That shows the formula is the derivative; tests/test_gpu_backdrop.py shows the kernels are the formula."""
import ctypes as C
import importlib
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

import backdrop_ref as BR
import coverage_ref as CR
import oracle_lib as O

S2D = importlib.import_module("2dgaussiansplatting_amd")
BACKDROP = importlib.import_module("2dgaussiansplatting_amd.backdrop")
HEADER = os.path.join(O.ROOT, "include", "splat2d_backdrop.h")
F32 = np.float32
E_INVALID = 1


# ---- the helper, pinned on its own -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "stack", "ones"])
@pytest.mark.parametrize("kind", ["constant", "plane"])
def test_a_black_backdrop_gives_the_plain_oracles_bytes(name, kind):
    tgt, s9 = BR.scene(name)
    H, W = tgt.shape[:2]
    black = np.zeros(3, dtype=F32) if kind == "constant" else np.zeros((H, W, 4), dtype=F32)
    plain = CR.oracle_of(tgt, s9)
    want = plain.forward().copy()
    wg, wsum, wabs = plain.backward_stats()
    b = BR.BackdropOracle(tgt, s9, black)
    got = b.forward()
    assert got.tobytes() == want.tobytes() and want[..., :3].any()
    g, dsum, dabs = b.backward_stats()
    assert g.tobytes() == wg.tobytes() and dsum.tobytes() == wsum.tobytes() and dabs.tobytes() == wabs.tobytes()
    assert b.T.shape == (H, W) and (b.T <= 1).all() and (b.T >= 0).all()


def test_without_splats_the_image_is_the_backdrop():
    tgt, s9 = BR.scene("empty")
    H, W = tgt.shape[:2]
    b = BR.BackdropOracle(tgt, s9, BR.CONSTANT)
    img = b.forward()
    assert (b.T == 1).all() and (img[..., :3] == BR.CONSTANT).all() and (img[..., 3] == 1).all()
    plane = BR.noise_plane(W, H)
    img = BR.BackdropOracle(tgt, s9, plane).forward()
    assert img[..., :3].tobytes() == np.ascontiguousarray(plane[..., :3]).tobytes() and (img[..., 3] == 1).all()


def test_the_scenes_are_not_trivial():
    """T_final exactly 1 and in (0.05, 0.95) on the 17 x 17 scene, below the 1/256 cut-off everywhere on the stack, exactly 0 on
    the opacity-1 scene; the deep stack has tiles with more than one batch of 64 entries' worth of splats over a pixel."""
    T = {k: BR.reference(k, "constant")[1] for k in ("tiny", "stack", "deep", "ones", "row")}
    assert (T["tiny"] == 1).any() and ((T["tiny"] > 0.05) & (T["tiny"] < 0.95)).any()
    assert (T["stack"] < 1.0 / 256.0).all() and (T["stack"] > 0).all()
    assert (T["ones"] == 0).any() and (T["ones"] == 1).any()
    assert (T["deep"] < 1.0 / 256.0).any() and len(BR.scene("deep")[1]) > 4 * 64
    assert T["row"].shape == (1, 200)
    for k in ("tiny", "deep", "row"):
        img, _, g, dsum, dabs = BR.reference(k, "plane")
        assert np.isfinite(img).all() and np.isfinite(g).all() and g.any()
    counts, variants = set(), set()
    for seed in BR.SWEEP_SEEDS:
        W, H, n, s, tgt = BR.sweep_case(seed)
        assert 36 <= W <= 289 and len(s) == n and tgt.shape == (H, W, 4)
        counts.add(n)
        variants.add(seed % 4)
    assert len(counts) >= 3 and variants == {0, 1, 2, 3}


# ---- the formula is the derivative ---------------------------------------------------------------------------------------------
def _fd_scene():
    """12 x 12, 6 splats that overlap each other and the image, no alpha near 1 (the scene of tests/test_coverage_cpu.py), with
    signed, spatially varying weights per channel."""
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
    w = np.stack([np.sin(0.9 * x + 0.4 * y + c) + 0.3 for c in range(3)], axis=-1)
    return s, W, H, w


def _fd_backdrops(W, H):
    rng = np.random.default_rng(77)
    return {"constant": np.array([1.0, 0.5, 0.25]), "plane": rng.uniform(0, 1, (H, W, 3))}


@pytest.mark.parametrize("kind", ["constant", "plane"])
@pytest.mark.parametrize("i", range(6))
def test_the_backward_expression_is_the_derivative_of_the_composite(i, kind):
    s, W, H, w = _fd_scene()
    B = _fd_backdrops(W, H)[kind]
    g = BR.composite_grads(s, W, H, w, B)
    assert np.abs(g).min() > 0
    # ... and the backdrop is at work in it: over black the geometric and opacity columns are others
    g0 = BR.composite_grads(s, W, H, w, np.zeros(3))
    assert np.abs(g - g0)[:, [0, 1, 2, 3, 4, 8]].min() > 1e-6 and np.array_equal(g[:, 5:8], g0[:, 5:8])
    loss = lambda s9: float(np.sum(w * BR.composite_of(s9, W, H, B)))
    h = 1e-6
    for k in range(9):
        sp, sm = s.copy(), s.copy()
        sp[i, k] += h
        sm[i, k] -= h
        fd = (loss(sp) - loss(sm)) / (2 * h)
        assert fd == pytest.approx(g[i, k], rel=1e-6, abs=1e-10), (i, k)   # tests/test_coverage_cpu.py, its scheme and its bar


def test_the_gradient_of_the_backdrop_is_the_throughput_times_the_upstream():
    s, W, H, w = _fd_scene()
    B = _fd_backdrops(W, H)["plane"]
    t = BR.backdrop_grads_of(s, W, H, w)
    loss = lambda b: float(np.sum(w * BR.composite_of(s, W, H, b)))
    for (y, x, c) in ((0, 0, 0), (5, 7, 1), (11, 3, 2), (6, 6, 0)):
        bp, bm = B.copy(), B.copy()
        bp[y, x, c] += 1e-3
        bm[y, x, c] -= 1e-3
        assert (loss(bp) - loss(bm)) / 2e-3 == pytest.approx(t[y, x, c], rel=1e-9, abs=1e-12)   # (linear in B: exact but for rounding)
    const = np.array([0.2, 0.9, 0.4])
    for c in range(3):
        bp, bm = const.copy(), const.copy()
        bp[c] += 1e-3
        bm[c] -= 1e-3
        lc = lambda b: float(np.sum(w * BR.composite_of(s, W, H, b)))
        assert (lc(bp) - lc(bm)) / 2e-3 == pytest.approx(t[..., c].sum(), rel=1e-9, abs=1e-12)


# ---- the surface ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    S2D._build.build_hip_library()
    L = S2D.load_library()
    BACKDROP.apply_backdrop_signatures(L)
    return L


def test_the_five_symbols_are_exported_and_the_header_compiles_as_c(lib, tmp_path):
    text = open(HEADER).read()
    assert BACKDROP.BACKDROP_SYMBOLS == ["s2d_set_backdrop", "s2d_set_backdrop_device", "s2d_get_backdrop", "s2d_throughput_device",
                                         "s2d_backdrop_grads"]
    for name in BACKDROP.BACKDROP_SYMBOLS:
        assert hasattr(lib, name) and name + "(" in text, name
    assert not set(BACKDROP.BACKDROP_SYMBOLS) & set(S2D.ABI_SYMBOLS)               # the pinned table of splat2d.h stays what it is
    assert "typedef" not in text and not re.search(r"\bstruct\s+\w*\s*\{", text)   # the header adds no structure
    assert "S2D_CFG_" not in re.sub(r"/\*.*?\*/", "", text, flags=re.S)             # ... and no configuration flag
    src = str(tmp_path / "c.c")
    with open(src, "w") as f:
        f.write('#include "splat2d_backdrop.h"\nint main(void) { int k; float c[3]; double d[3];\n'
                '  return s2d_set_backdrop(0, c) + s2d_set_backdrop_device(0, 0) + s2d_get_backdrop(0, &k, c) + s2d_throughput_device(0, 0)\n'
                '         + s2d_backdrop_grads(0, 0, 0, d) == 5 * S2D_E_INVALID ? 0 : 1; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(O.ROOT, "include"), src])


def test_the_bindings_table_is_the_header(lib):
    """Every declaration of the header, in its order, is an entry of the table with as many arguments, all of them pointers
    (void pointers to ctypes), returning int."""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    decls = re.findall(r"^\s*(\w[\w\s\*]*?)\b(s2d_\w+)\s*\(([^)]*)\)\s*;", src, flags=re.M)
    assert [d[1] for d in decls] == BACKDROP.BACKDROP_SYMBOLS
    for ret, name, params in decls:
        argtypes, restype = BACKDROP.BACKDROP_SIGNATURES[name]
        ps = [p.strip() for p in params.split(",")]
        assert ret.strip() == "int" and restype is C.c_int, name
        assert len(ps) == len(argtypes) and all("*" in p or "[" in p for p in ps) and all(t is C.c_void_p for t in argtypes), name
        f = getattr(lib, name)
        assert list(f.argtypes) == argtypes and f.restype is restype


def test_backdrop_trainer_has_its_methods_and_no_torch():
    T = S2D.BackdropTrainer
    assert T is BACKDROP.BackdropTrainer and issubclass(T, S2D.Trainer)
    own = sorted(n for n, v in vars(T).items() if callable(v) and not n.startswith("_"))
    assert set(own) >= {"set_backdrop", "set_backdrop_device", "backdrop", "throughput", "throughput_device", "backdrop_grads"}
    assert set(own) - {"set_backdrop", "set_backdrop_device", "backdrop", "throughput", "throughput_device", "backdrop_grads"} == \
        {"set_backdrop_plane", "backdrop_plane_grads", "of"}   # the host conveniences around the two device calls; a Trainer adopted
    assert "torch" not in open(BACKDROP.__file__).read().replace("No torch", "").replace("torch_backdrop", "")


def _have_hipcc():
    try:
        return bool(S2D._build.hipcc())
    except RuntimeError:
        return False


@pytest.mark.skipif(not _have_hipcc(), reason="hipcc is not installed: the unit cannot be cross-compiled")
def test_the_unit_emits_its_fourteen_kernels_without_scratch():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(O.ROOT, "tools", "kernel_resources.py"))
    KR = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(KR)
    got = KR.report(os.path.join(O.ROOT, "2dgaussiansplatting_amd", "csrc"), "s2d_backdrop.hip")
    tf = ("false", "true")
    want = sorted(["s2d::backdrop_forward_kernel<%s, %s>" % (h, p) for h in tf for p in tf] +
                  ["s2d::backdrop_view_kernel<%d, %s>" % (s, r) for s in (1, 2, 4) for r in tf] +
                  ["s2d::backdrop_grad_kernel<false, false>", "s2d::backdrop_grad_kernel<true, false>",
                   "s2d::backdrop_grad_kernel<false, true>", "s2d::backdrop_grad_finish_kernel"])
    assert len(want) == 14 and sorted(got) == want
    for name, r in got.items():
        assert r["scratch"] == 0 and r["agprs"] == 0, (name, r)
        assert not re.match(r"s2d::(raster_|view_raster_kernel|view_gradient_kernel)", name)   # the prefixes the variant tables pin
        if "forward" in name or "view" in name:
            assert r["vgprs"] <= 64 and r["occupancy"] == 8, (name, r)


# ---- refusals that need no device ------------------------------------------------------------------------------------------------
def _config(flags=0, W=64, H=64, row_begin=0, row_end=0):
    cfg = S2D._Config()
    cfg.struct_size = C.sizeof(S2D._Config)
    cfg.width, cfg.height, cfg.n_splats = W, H, 10
    cfg.row_begin, cfg.row_end = row_begin, row_end
    cfg.flags = flags
    return cfg


class _Context:
    """A context as s2d_create hands it out: whole where there is a device, and without one still a handle that explains itself
    (rc S2D_E_HIP) -- what the setters refuse for the configuration they refuse on either."""

    def __init__(self, lib, **kw):
        self.lib, self.h = lib, C.c_void_p()
        cfg = _config(**kw)
        self.rc = lib.s2d_create(C.byref(cfg), C.byref(self.h))
        assert self.rc in (0, 2) and self.h.value

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.lib.s2d_destroy(self.h)

    def error(self):
        return self.lib.s2d_last_error(self.h).decode()


def test_null_handles_and_null_outputs(lib):
    rgb = (C.c_float * 3)(1, 1, 1)
    kind = C.c_int(7)
    assert lib.s2d_set_backdrop(None, rgb) == E_INVALID and lib.s2d_set_backdrop_device(None, None) == E_INVALID
    assert lib.s2d_get_backdrop(None, C.byref(kind), rgb) == E_INVALID and lib.s2d_throughput_device(None, None) == E_INVALID
    assert lib.s2d_backdrop_grads(None, None, None, None) == E_INVALID


@pytest.mark.parametrize("flag", ["S2D_CFG_COVERAGE", "S2D_CFG_COUNT_PAIRS", "S2D_CFG_EXACT_EXP", "S2D_CFG_REFERENCE_ORDER"])
def test_the_setters_refuse_the_contexts_without_kernels(lib, flag):
    rgb = (C.c_float * 3)(1, 1, 1)
    with _Context(lib, flags=getattr(S2D, flag)) as c:
        assert lib.s2d_set_backdrop(c.h, rgb) == E_INVALID and flag in c.error() and "s2d_set_backdrop" in c.error()
        assert lib.s2d_set_backdrop_device(c.h, C.c_void_p(4096)) == E_INVALID and flag in c.error()
        kind = C.c_int(7)
        assert lib.s2d_get_backdrop(c.h, C.byref(kind), rgb) == 0 and kind.value == 0 and list(rgb) == [0, 0, 0]


def test_the_setters_refuse_a_slab_context_and_bad_arguments(lib):
    rgb = (C.c_float * 3)(1, 1, 1)
    with _Context(lib, row_begin=16, row_end=48) as c:
        assert lib.s2d_set_backdrop(c.h, rgb) == E_INVALID and "slab" in c.error()
        assert lib.s2d_set_backdrop_device(c.h, C.c_void_p(4096)) == E_INVALID and "slab" in c.error()
    with _Context(lib) as c:
        for bad in (float("nan"), float("inf"), -float("inf")):
            for k in range(3):
                v = (C.c_float * 3)(0.5, 0.5, 0.5)
                v[k] = bad
                assert lib.s2d_set_backdrop(c.h, v) == E_INVALID and "finite" in c.error()
        assert lib.s2d_set_backdrop_device(c.h, None) == E_INVALID and "NULL" in c.error()
        assert lib.s2d_set_backdrop_device(c.h, C.c_void_p(4096 + 8)) == E_INVALID and "aligned" in c.error()
        assert lib.s2d_set_backdrop(c.h, None) == 0                     # nothing to remove: nothing to do
        kind = C.c_int(7)
        assert lib.s2d_get_backdrop(c.h, C.byref(kind), None) == 0 and kind.value == 0
        assert lib.s2d_get_backdrop(c.h, None, None) == E_INVALID
        # without a backdrop there is no throughput plane and no gradient of one
        assert lib.s2d_throughput_device(c.h, C.c_void_p(4096)) == E_INVALID and "no backdrop" in c.error()
        assert lib.s2d_throughput_device(c.h, None) == E_INVALID
        assert lib.s2d_backdrop_grads(c.h, None, C.c_void_p(4096), None) == E_INVALID and "no backdrop" in c.error()
        assert lib.s2d_backdrop_grads(c.h, C.c_void_p(4096 + 4), None, None) == E_INVALID and "aligned" in c.error()


def test_the_trainer_checks_the_shape_of_a_constant():
    t = S2D.BackdropTrainer.__new__(S2D.BackdropTrainer)   # (no context: the refusal stands in front of it)
    t._h = None
    for bad in ([1.0, 1.0], [[1.0, 1.0, 1.0]], 1.0):
        with pytest.raises(S2D.S2DError) as ei:
            t.set_backdrop(bad)
        assert ei.value.code == E_INVALID


# ---- the host tool's argument errors (all of them in front of s2d_create: no device is asked for) -------------------------------
BAD_ARGS = [
    (["--background", "1,1"], "R,G,B"), (["--background", "1,1,1,1"], "R,G,B"), (["--background", "a,b,c"], "R,G,B"),
    (["--background", ""], "R,G,B"), (["--background", "1,1,"], "R,G,B"), (["--background", "nan,0,0"], "R,G,B"),
    (["--background", "0,inf,0"], "R,G,B"), (["--background", "1 1 1"], "R,G,B"),
    (["--background", "1,1,1", "--coverage"], "--background"), (["--background", "1,1,1", "--gpus", "2"], "--background"),
    (["--background", "1,1,1", "--reference-order"], "--background"), (["--background", "1,1,1", "--coarse", "0.5:3"], "--background"),
]


@pytest.mark.parametrize("args,word", BAD_ARGS, ids=[" ".join(a) for a, _ in BAD_ARGS])
def test_host_tool_refuses_bad_background_arguments(lib, args, word):
    train = S2D._build.build_host_program()
    r = subprocess.run([train, "--synthetic", "32x32", "--splats", "4", "--iters", "4"] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and word in r.stderr, (r.returncode, r.stderr[-500:])
    assert "no CPU fallback" not in r.stderr and "s2d_create" not in r.stderr and r.stdout == ""


def test_host_tool_help_says_a_checkpoint_does_not_carry_the_background(lib):
    train = S2D._build.build_host_program()
    r = subprocess.run([train, "--help"], capture_output=True, text=True, timeout=60)
    assert "--background R,G,B" in r.stderr and re.search(r"checkpoint does not carry the background", r.stderr)
