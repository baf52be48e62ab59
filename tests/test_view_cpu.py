"""CPU tests of view rendering's shared arithmetic: csrc/s2d_view_math.h compiled for the host (tests/hostcheck/
s2d_view_check.cpp) against the NumPy restatement tests/view_ref.py, byte for byte."""
import ctypes as C
import importlib

import numpy as np
import pytest

import oracle_lib as O
import view_hostcheck
import view_ref as V

S2D = importlib.import_module("2dgaussiansplatting_amd")
F = np.float32


@pytest.fixture(scope="module")
def hc():
    return view_hostcheck.load()


def host_rows(hc, splats, origin, zoom, filter_var, samples):
    out = np.zeros(len(splats), dtype=O.SPLAT_DTYPE)
    hc.vc_rows(O._p(splats), len(splats), origin[0], origin[1], zoom, filter_var, samples, O._p(out))
    return out


@pytest.fixture(scope="module")
def records():
    """10^5 records over the ranges the library accepts, with a few zeros, negatives and non-finite values among them."""
    rng = np.random.default_rng(2024)
    n = 100000
    s = np.zeros(n, dtype=O.SPLAT_DTYPE)
    s["pos"] = rng.uniform(-50, 4200, (n, 2))
    s["sx"] = np.exp(rng.uniform(np.log(0.01), np.log(2000.0), n))
    s["sy"] = np.exp(rng.uniform(np.log(0.01), np.log(2000.0), n))
    s["rot"] = rng.uniform(-7, 7, n)
    s["color"] = rng.uniform(-0.5, 1.5, (n, 3))
    s["opacity"] = rng.uniform(0, 1, n)
    s["sx"][:4] = [0.0, -3.0, np.inf, np.nan]
    s["sy"][4:8] = [0.0, -0.0, 1e-30, 1e30]
    s["pos"][8:10, 0] = [np.nan, -np.inf]
    s["opacity"][10:12] = [np.nan, -0.0]
    return s


@pytest.mark.parametrize("samples", [1, 2, 4])
@pytest.mark.parametrize("view", V.VIEWS, ids=V.VIEW_IDS)
def test_transform_equals_numpy(hc, records, view, samples):
    origin, zoom, fv, _ = view
    got = host_rows(hc, records, origin, zoom, fv, samples)
    want = V.view_rows(records, origin, zoom, fv, samples)
    assert got.tobytes() == want.tobytes()


def test_samples_zero_means_one(hc, records):
    origin, zoom, fv, _ = V.VIEWS[2]
    assert host_rows(hc, records, origin, zoom, fv, 0).tobytes() == host_rows(hc, records, origin, zoom, fv, 1).tobytes()
    assert V.view_rows(records, origin, zoom, fv, 0).tobytes() == V.view_rows(records, origin, zoom, fv, 1).tobytes()


def test_identity_view_keeps_the_bytes(hc, records):
    assert host_rows(hc, records, (0.0, 0.0), 1.0, 0.0, 1).tobytes() == records.tobytes()
    assert V.view_rows(records, (0.0, 0.0), 1.0, 0.0, 1).tobytes() == records.tobytes()


def test_views_of_scene_m_stay_in_the_pinned_range():
    m = V.scene_m()
    for origin, zoom, fv, _ in V.VIEWS:
        assert V.scales_in_pinned_range(V.view_rows(m, origin, zoom, fv, 1))


def test_config_size_matches_ctypes(hc):
    assert hc.vc_config_size() == C.sizeof(S2D._ViewConfig) == 36


@pytest.mark.parametrize("changes,refused", V.REFUSAL_TABLE, ids=[str(k) for k in range(len(V.REFUSAL_TABLE))])
def test_refusal_predicate(hc, changes, refused):
    cfg = V.make_config(S2D._ViewConfig, **dict(changes))
    assert bool(hc.vc_refused(C.byref(cfg))) == refused


def test_resolve_equals_numpy(hc):
    rng = np.random.default_rng(5)
    img = rng.uniform(-0.5, 1.5, (48, 80, 4)).astype(F)
    img[3, 5, 0], img[4, 4, 1], img[0, 0, 2] = np.nan, np.inf, -0.0
    img[10:14, 20:24, :3] = F(1e-42)  # denormals
    got = np.zeros((24, 40, 4), dtype=F)
    hc.vc_resolve2(O._p(img), 40, 24, O._p(got))
    want = V.resolve(img, 2)
    assert got.tobytes() == want.tobytes()
    got4 = np.zeros((12, 20, 4), dtype=F)
    hc.vc_resolve2(O._p(got), 20, 12, O._p(got4))
    assert got4.tobytes() == V.resolve(img, 4).tobytes()
    assert V.resolve(img, 1) is img


def test_quantiser_equals_numpy(hc):
    k = np.arange(256, dtype=F) / F(255.0)
    edges = (np.arange(256, dtype=F) - F(0.5)) / F(255.0)  # where the rounding flips
    vals = np.concatenate([k, np.nextafter(k, F(-np.inf)), np.nextafter(k, F(np.inf)),
                           edges, np.nextafter(edges, F(-np.inf)), np.nextafter(edges, F(np.inf)),
                           np.array([np.nan, -np.nan, np.inf, -np.inf, -0.0, 0.0, -0.2, 1.5, 1.0, 1e-45, -1e-45, 3e38, 0.5], dtype=F)])
    vals = np.concatenate([vals, np.zeros((-len(vals)) % 3, dtype=F)])
    img = np.zeros((len(vals) // 3, 4), dtype=F)
    img[:, :3] = vals.reshape(-1, 3)
    got = np.zeros(len(img), dtype=np.uint32)
    hc.vc_quantise(O._p(img), len(img), O._p(got))
    want = V.quantise(img)
    assert got.view(np.uint8).reshape(-1, 4).tobytes() == want.tobytes()
    # every k / 255 comes back as k
    img2 = np.zeros((256, 4), dtype=F)
    img2[:, 0] = k
    assert np.array_equal(V.quantise(img2)[:, 0], np.arange(256, dtype=np.uint8))
    assert np.array_equal(V.quantise(np.array([[np.nan, -0.2, 1.5, 0]], dtype=F))[0], np.array([0, 0, 255, 255], dtype=np.uint8))
