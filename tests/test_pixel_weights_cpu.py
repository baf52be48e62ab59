"""CPU tests of the pixel-weight plane (include/splat2d_weights.h): the two yardsticks of
tests/weights_ref.py against each other and, with a plane of ones, against tests/loss_ref.py; and the surface -- the header as C,
the four exported symbols, the binding's table against the header, the structure's layout, the kernels the new unit emits, the
refusals that need no device and the argument errors of `splat2d_train --weight-image`.  No GPU.

That the torch evaluation (autograd through conv2d) and the NumPy one (the adjoint by hand, the plane at the window's centre)
agree shows the formula of the header is the derivative of L_omega; tests/test_gpu_pixel_weights.py shows the kernels are the
formula."""
import ctypes as C
import importlib
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

import loss_ref as LR
import oracle_lib as O
import weights_ref as WR

S2D = importlib.import_module("2dgaussiansplatting_amd")
WEIGHTS = importlib.import_module("2dgaussiansplatting_amd.weights")
HEADER = os.path.join(O.ROOT, "include", "splat2d_weights.h")
E_INVALID = 1
ALL_WEIGHTINGS = WR.WEIGHTINGS + [(0.0, 0.0, 1.0), (0.0, 1.0, 0.0)]


# ---- the two yardsticks ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["random", "mask"])
@pytest.mark.parametrize("size", sorted(WR.SIZES))
def test_autograd_and_the_hand_derived_adjoint_agree(size, kind):
    W, H = WR.SIZES[size]
    om = WR.plane(kind, W, H, seed=W)
    for content in ("noise", "smooth"):
        x, y = WR.image_pair(W, H, content, 7 + W)
        for w in ALL_WEIGHTINGS:
            a, b = WR.torch_wloss(x, y, om, w), WR.numpy_wloss(x, y, om, w)
            big = np.abs(a["grad"]).max()
            assert big > 0
            assert np.abs(a["grad"] - b["grad"]).max() <= 1e-12 * big, (size, kind, content, w)
            for k in ("mse", "wmse", "l1", "dssim", "total", "weight_sum"):
                if a[k] is None:
                    assert b[k] is None
                else:
                    assert a[k] == pytest.approx(b[k], rel=1e-12, abs=1e-15), (size, kind, content, w, k)
            if kind == "mask" and w[2] == 0:    # without the window a masked pixel has no gradient at all
                assert not a["grad"][om == 0].any() and not b["grad"][om == 0].any()


def test_the_dssim_weight_sits_at_the_window_centre():
    """A masked pixel within the window's reach of a counted one still has a D-SSIM gradient; one further away has none; and
    weighting the unweighted gradient image afterwards (omega * g) is another function."""
    W, H = 96, 80
    om = np.zeros((H, W), dtype=np.float32)
    om[:, 48:] = 1.0
    x, y = WR.image_pair(W, H, "noise", 3)
    w = (0.0, 0.0, 1.0)
    g = WR.numpy_wloss(x, y, om, w)["grad"]
    assert not g[:, :43].any() and np.abs(g[:, 43:48]).min(axis=2).max() > 0
    plain = LR.numpy_loss(x, y, w)["grad"]
    assert np.abs(g - om[..., None] * plain).max() > 1e-3 * np.abs(plain).max()


@pytest.mark.parametrize("size", sorted(WR.SIZES))
def test_a_plane_of_ones_reproduces_loss_ref_exactly(size):
    W, H = WR.SIZES[size]
    x, y = WR.image_pair(W, H, "noise", 11)
    ones = WR.plane("ones", W, H)
    for w in ALL_WEIGHTINGS:
        for weighted, plain in ((WR.torch_wloss(x, y, ones, w), LR.torch_loss(x, y, w)), (WR.numpy_wloss(x, y, ones, w), LR.numpy_loss(x, y, w)),
                                (WR.torch_wloss(x, y, ones, w, "float32"), LR.torch_loss(x, y, w, "float32"))):
            assert weighted["grad"].tobytes() == plain["grad"].tobytes(), (size, w)
            assert weighted["mse"] == plain["mse"] == weighted["wmse"]
            assert weighted["l1"] == plain["l1"] and weighted["dssim"] == plain["dssim"] and weighted["total"] == plain["total"]
            assert weighted["weight_sum"] == W * H


def test_the_planes_are_what_the_tests_need():
    for size, (W, H) in WR.SIZES.items():
        r, m = WR.plane("random", W, H, seed=W), WR.plane("mask", W, H)
        assert r.dtype == m.dtype == np.float32 and r.shape == m.shape == (H, W)
        assert r.min() >= 0 and r.max() <= 2 and set(np.unique(m)) == {0.0, 1.0}
    m = WR.plane("mask", 96, 80)
    assert m[:, 31].any() and not m[:, 32:].any()              # the edge at x = 32, the border of two loss tiles
    assert not m[40:, :16].any() and m[40:, 16:32].all()       # ... and the one inside a tile
    x, y = WR.image_pair(33, 17, "noise", 1)
    s, wsq, wl1 = WR.weighted_sums_exact(x, y, np.ones((17, 33), dtype=np.float32))
    assert s == 33 * 17 and wsq == LR.sqerr255_exact(x, y) and wl1 > 0


# ---- the surface ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    S2D._build.build_hip_library()
    L = S2D.load_library()
    WEIGHTS.apply_weights_signatures(L)
    return L


def test_the_four_symbols_are_exported_and_the_header_compiles_as_c(lib, tmp_path):
    text = open(HEADER).read()
    assert WEIGHTS.WEIGHTS_SYMBOLS == ["s2d_set_pixel_weights", "s2d_set_pixel_weights_device", "s2d_get_pixel_weights", "s2d_weighted_loss_get"]
    for name in WEIGHTS.WEIGHTS_SYMBOLS:
        assert hasattr(lib, name) and name + "(" in text, name
    assert not set(WEIGHTS.WEIGHTS_SYMBOLS) & set(S2D.ABI_SYMBOLS)                   # the pinned table of splat2d.h stays what it is
    assert "S2D_CFG_" not in re.sub(r"/\*.*?\*/", "", text, flags=re.S)               # no configuration flag
    assert "s2d_set_pixel_weights(ctx, NULL)" in text
    src = str(tmp_path / "c.c")
    with open(src, "w") as f:
        f.write('#include <stddef.h>\n#include "splat2d_weights.h"\n'
                '_Static_assert(sizeof(s2d_weighted_terms) == 48, "size");\n'
                '_Static_assert(offsetof(s2d_weighted_terms, weight_sum) == 8 && offsetof(s2d_weighted_terms, total) == 40, "layout");\n'
                'int main(void) { int32_t k; double d; s2d_weighted_terms t = { sizeof t, 0, 0, 0, 0, 0, 0 };\n'
                '  return s2d_set_pixel_weights(0, 0) + s2d_set_pixel_weights_device(0, 0) + s2d_get_pixel_weights(0, &k, &d, 0)\n'
                '         + s2d_weighted_loss_get(0, &t) == 4 * S2D_E_INVALID ? 0 : 1; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(O.ROOT, "include"), src])


def test_the_bindings_table_is_the_header(lib):
    """Every declaration of the header, in its order, is an entry of the table with as many arguments, all of them pointers,
    returning int; the one structure has the header's fields."""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    decls = re.findall(r"^\s*(\w[\w\s\*]*?)\b(s2d_\w+)\s*\(([^)]*)\)\s*;", src, flags=re.M)
    assert [d[1] for d in decls] == WEIGHTS.WEIGHTS_SYMBOLS
    for ret, name, params in decls:
        argtypes, restype = WEIGHTS.WEIGHTS_SIGNATURES[name]
        ps = [p.strip() for p in params.split(",")]
        assert ret.strip() == "int" and restype is C.c_int, name
        assert len(ps) == len(argtypes) and all("*" in p for p in ps), name
        for p, t in zip(ps, argtypes):
            assert t is (C.POINTER(WEIGHTS._WeightedTerms) if "s2d_weighted_terms" in p else C.c_void_p), (name, p)
        f = getattr(lib, name)
        assert list(f.argtypes) == argtypes and f.restype is restype
    body = re.search(r"typedef struct s2d_weighted_terms \{(.*?)\} s2d_weighted_terms;", src, flags=re.S).group(1)
    fields = []
    for ctype, names in re.findall(r"(uint32_t|double)\s+([\w\s,]+);", body):
        fields += [(n.strip(), ctype) for n in names.split(",")]
    T = WEIGHTS._WeightedTerms
    assert fields == [(n, "uint32_t" if t is C.c_uint32 else "double") for n, t in T._fields_]
    assert [n for n, _ in T._fields_] == ["struct_size", "reserved", "weight_sum", "mse", "l1", "dssim", "total"]
    assert C.sizeof(T) == 48 and T.weight_sum.offset == 8 and T.total.offset == 40


def test_weighted_trainer_has_its_methods_and_no_torch():
    T = S2D.WeightedTrainer
    assert T is WEIGHTS.WeightedTrainer and issubclass(T, S2D.Trainer) and "WeightedTrainer" in S2D.__all__
    own = sorted(n for n, v in vars(T).items() if (callable(v) or isinstance(v, staticmethod)) and not n.startswith("_"))
    assert own == ["of", "pixel_weights", "set_pixel_weights", "set_pixel_weights_device", "weighted_terms"]
    assert "torch" not in open(WEIGHTS.__file__).read().replace("No torch", "")
    with pytest.raises(S2D.S2DError) as ei:
        T.of(object())                                                           # (the multi-device handle among them)
    assert ei.value.code == E_INVALID


def _have_hipcc():
    try:
        return bool(S2D._build.hipcc())
    except RuntimeError:
        return False


@pytest.mark.skipif(not _have_hipcc(), reason="hipcc is not installed: the unit cannot be cross-compiled")
def test_the_unit_cross_compiles_for_gfx950_without_scratch():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(O.ROOT, "tools", "kernel_resources.py"))
    KR = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(KR)
    assert "s2d_loss_weighted.hip" in S2D._build.HIP_SOURCES and "s2d_loss_weighted.h" in S2D._build.HIP_HEADERS
    got = KR.report(os.path.join(O.ROOT, "2dgaussiansplatting_amd", "csrc"), "s2d_loss_weighted.hip")
    want = sorted(["s2d::wloss_%s_kernel<%s>" % (k, h) for k in ("moments", "adjoint", "pointwise") for h in ("false", "true")] +
                  ["s2d::wloss_finalize_kernel", "s2d::weight_check_kernel", "s2d::weight_check_finish_kernel"])
    assert sorted(got) == want
    for name, r in got.items():
        assert r["scratch"] == 0 and r["agprs"] == 0, (name, r)
        assert not re.match(r"s2d::(raster_|view_raster_kernel|view_gradient_kernel)", name)   # the prefixes the variant tables pin
    for h in ("false", "true"):                                                   # three waves per SIMD, as the unweighted window kernels
        assert got["s2d::wloss_adjoint_kernel<%s>" % h]["occupancy"] >= 3 and got["s2d::wloss_moments_kernel<%s>" % h]["occupancy"] >= 3


# ---- statuses that need no device ------------------------------------------------------------------------------------------------
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


def _terms():
    t = WEIGHTS._WeightedTerms()
    t.struct_size = C.sizeof(t)
    return t


def test_null_handles_and_null_outputs(lib):
    plane = (C.c_float * 4)(1, 1, 1, 1)
    k, d, t = C.c_int32(7), C.c_double(), _terms()
    assert lib.s2d_set_pixel_weights(None, plane) == E_INVALID and lib.s2d_set_pixel_weights(None, None) == E_INVALID
    assert lib.s2d_set_pixel_weights_device(None, C.c_void_p(4096)) == E_INVALID
    assert lib.s2d_get_pixel_weights(None, C.byref(k), C.byref(d), None) == E_INVALID
    assert lib.s2d_weighted_loss_get(None, C.byref(t)) == E_INVALID
    with _Context(lib) as c:
        assert lib.s2d_get_pixel_weights(c.h, None, None, None) == E_INVALID
        assert lib.s2d_weighted_loss_get(c.h, None) == E_INVALID


@pytest.mark.parametrize("flag", ["S2D_CFG_COVERAGE", "S2D_CFG_COUNT_PAIRS"])
def test_the_setters_refuse_the_contexts_without_a_loss_pass(lib, flag):
    plane = (C.c_float * (64 * 64))(*([1.0] * (64 * 64)))
    with _Context(lib, flags=getattr(S2D, flag)) as c:
        assert lib.s2d_set_pixel_weights(c.h, plane) == E_INVALID and flag in c.error() and "s2d_set_pixel_weights" in c.error()
        assert lib.s2d_set_pixel_weights_device(c.h, C.c_void_p(4096)) == E_INVALID and flag in c.error()
        k, d = C.c_int32(7), C.c_double(7)
        assert lib.s2d_get_pixel_weights(c.h, C.byref(k), C.byref(d), None) == 0 and k.value == 0 and d.value == 0.0


def test_the_setters_refuse_a_slab_context_and_bad_arguments(lib):
    plane = (C.c_float * (64 * 64))(*([1.0] * (64 * 64)))
    with _Context(lib, row_begin=16, row_end=48) as c:     # (what a rank of the multi-device handle is)
        assert lib.s2d_set_pixel_weights(c.h, plane) == E_INVALID and "slab" in c.error()
        assert lib.s2d_set_pixel_weights_device(c.h, C.c_void_p(4096)) == E_INVALID and "slab" in c.error()
    with _Context(lib) as c:
        assert lib.s2d_set_pixel_weights_device(c.h, C.c_void_p(4096 + 8)) == E_INVALID and "aligned" in c.error()
        assert lib.s2d_set_pixel_weights(c.h, None) == 0 and lib.s2d_set_pixel_weights_device(c.h, None) == 0   # nothing to remove
        k, d = C.c_int32(7), C.c_double(7)
        assert lib.s2d_get_pixel_weights(c.h, C.byref(k), None, None) == 0 and k.value == 0
        assert lib.s2d_get_pixel_weights(c.h, C.byref(k), C.byref(d), plane) == 0 and d.value == 0.0 and plane[0] == 1.0
        t = _terms()
        assert lib.s2d_weighted_loss_get(c.h, C.byref(t)) == E_INVALID and "no pixel weights" in c.error()
        t.struct_size -= 8
        assert lib.s2d_weighted_loss_get(c.h, C.byref(t)) == E_INVALID and "struct_size" in c.error()


def test_the_trainer_checks_the_shape_of_a_plane():
    t = S2D.WeightedTrainer.__new__(S2D.WeightedTrainer)   # (no context: the refusal stands in front of it)
    t._h, t.W, t.H = None, 8, 4
    for bad in (np.ones((8, 4)), np.ones(32), np.ones((4, 8, 1)), 1.0):
        with pytest.raises(S2D.S2DError) as ei:
            t.set_pixel_weights(bad)
        assert ei.value.code == E_INVALID


# ---- the host tool's argument errors (all of them in front of s2d_create: no device is asked for) -------------------------------
def _write_ppm(path, W, H, value):
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (W, H) + bytes([value]) * (3 * W * H))


BAD_ARGS = [
    (["--weight-gain", "2"], "--weight-image"), (["--weight-image", "W", "--weight-gain", "-1"], "--weight-gain"),
    (["--weight-image", "W", "--weight-gain", "abc"], "--weight-gain"), (["--weight-image", "W", "--weight-gain", "nan"], "--weight-gain"),
    (["--weight-image", "W", "--weight-gain", "1x"], "--weight-gain"), (["--weight-image", "W", "--gpus", "2"], "--weight-image"),
    (["--weight-image", "W", "--coverage"], "--weight-image"), (["--weight-image", "W", "--coarse", "0.5:3"], "--weight-image"),
    (["--weight-image", "missing.ppm"], "cannot read the weight image"), (["--weight-image", "SMALL"], "needs the target's size"),
]


@pytest.mark.parametrize("args,word", BAD_ARGS, ids=[" ".join(a) for a, _ in BAD_ARGS])
def test_host_tool_refuses_bad_weight_arguments(lib, tmp_path, args, word):
    train = S2D._build.build_host_program()
    good, small = str(tmp_path / "w.ppm"), str(tmp_path / "small.ppm")
    _write_ppm(good, 32, 32, 255)
    _write_ppm(small, 16, 32, 255)
    args = [{"W": good, "SMALL": small, "missing.ppm": str(tmp_path / "missing.ppm")}.get(a, a) for a in args]
    r = subprocess.run([train, "--synthetic", "32x32", "--splats", "4", "--iters", "4"] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode in (1, 2) and word in r.stderr, (r.returncode, r.stderr[-500:])
    assert "no CPU fallback" not in r.stderr and "s2d_create" not in r.stderr and r.stdout == ""


def test_host_tool_help_says_a_checkpoint_does_not_carry_the_plane(lib):
    train = S2D._build.build_host_program()
    r = subprocess.run([train, "--help"], capture_output=True, text=True, timeout=60)
    assert "--weight-image file" in r.stderr and "--weight-gain G" in r.stderr and "provisional" in r.stderr
    assert re.search(r"checkpoint does not carry the weight plane", r.stderr)
