"""CPU tests of the relocation planner behind s2d_relocate (2dgaussiansplatting_amd/csrc/s2d_density.h).

tests/hostcheck/s2d_density_check.cpp compiles the planner -- the function the library itself calls -- for the host.  Here
it is held, on bits, to a NumPy restatement of its four rules (the header's comment) that shares nothing with it but
`sincos_f32`, taken through the existing host shim (tests/hostcheck/s2d_hostcheck.cpp): every other operation is a single
binary32 or binary64 operation that NumPy rounds the same way.  The same planner behind a main() of its own
(tests/hostcheck/s2d_density_main.cpp) is built with -fsanitize=address,undefined and run as a child process on the edge
inputs; nothing sanitised is loaded into Python.

This module is also where tests/test_gpu_density.py takes the planner shim from.
"""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import oracle_lib as O

HERE = os.path.dirname(os.path.abspath(__file__))
HC_DIR = os.path.join(HERE, "hostcheck")
CSRC = os.path.join(O.ROOT, "2dgaussiansplatting_amd", "csrc")
F32 = np.float32
INF = float("inf")


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _shim(name, source, deps, extra=()):
    so = os.path.join(HC_DIR, name)
    srcs = [os.path.join(HC_DIR, source)] + deps
    if not os.path.exists(so) or any(os.path.getmtime(so) < os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-std=c++17", "-I", os.path.join(O.ROOT, "include"),
                               "-o", so, srcs[0], "-lm"] + list(extra))
    return C.CDLL(so)


_planner = None


def planner():
    """ctypes handle of the planner shim (built on demand)."""
    global _planner
    if _planner is None:
        L = _shim("libs2d_density_check.so", "s2d_density_check.cpp", [os.path.join(CSRC, "s2d_density.h"), os.path.join(CSRC, "s2d_math.h")])
        L.dp_plan.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                              C.c_void_p]
        L.dp_plan.restype = C.c_int
        _planner = L
    return _planner


def plan(stats, passes, max_moves, min_weight, shrink, W, H, splats9, adams18):
    """The planner on copies of the arrays -> (ids [moves, 2] (donor, starved), splats (n, 9), adams (n, 18))."""
    n = len(splats9)
    st = np.ascontiguousarray(stats, dtype=F32).reshape(n, 3)
    s = np.array(splats9, dtype=F32).reshape(n, 9).copy()
    a = np.array(adams18, dtype=F32).reshape(n, 18).copy()
    ids = np.full(2 * max(min(int(max_moves), n), 0) + 1, -1, dtype=np.int32)
    moves = planner().dp_plan(n, _p(st), int(passes), int(max_moves), float(min_weight), float(shrink), int(W), int(H), _p(s), _p(a), _p(ids))
    assert 0 <= 2 * moves < len(ids) and np.all(ids[2 * moves:] == -1)
    return ids[:2 * moves].reshape(-1, 2).copy(), s, a


@pytest.fixture(scope="module")
def sincos():
    L = _shim("libs2d_hostcheck.so", "s2d_hostcheck.cpp",
              [os.path.join(CSRC, "s2d_math.h"), os.path.join(O.ROOT, "2dgaussiansplatting_amd", "host", "overlay.h")], extra=("-lz",))
    L.hc_sincos.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.hc_sincos.restype = None

    def f(x):
        x = np.ascontiguousarray(x, dtype=F32)
        s, c = np.zeros_like(x), np.zeros_like(x)
        L.hc_sincos(_p(x), len(x), _p(s), _p(c))
        return s, c
    return f


def clamp(x, lo, hi):
    t = lo if x < lo else x       # glm::clamp, main.cpp:741-745
    return hi if hi < t else t


def plan_numpy(stats, passes, max_moves, min_weight, shrink, W, H, splats9, adams18, sincos):
    """Rules 1-4 of s2d_density.h, restated."""
    n = len(splats9)
    s = np.array(splats9, dtype=F32).reshape(n, 9).copy()
    a = np.array(adams18, dtype=F32).reshape(n, 18).copy()
    if n == 0 or passes <= 0 or max_moves <= 0:
        return np.zeros((0, 2), dtype=np.int32), s, a
    st = np.asarray(stats, dtype=F32).reshape(n, 3).astype(np.float64)
    w = st[:, 2] / float(passes)                                    # rule 1, in double
    mag = np.hypot(st[:, 0], st[:, 1]) / float(passes)
    is_starved = w < np.float64(F32(min_weight))
    starved = sorted(np.nonzero(is_starved)[0], key=lambda i: (w[i], i))[:max_moves]           # rule 2
    donors = sorted(np.nonzero(~is_starved & (mag > 0))[0], key=lambda i: (-mag[i], i))         # rule 3
    m = min(len(starved), len(donors))
    sn, cs = sincos(s[:, 4])
    ids = []
    for d, t in zip(donors[:m], starved[:m]):                       # rule 4, every operation in binary32
        sx, sy = s[d, 2], s[d, 3]
        along_x = not (sx < sy)
        sigma = clamp((sx if along_x else sy) / F32(shrink), F32(1), F32(1024))
        ux, uy = (cs[d], sn[d]) if along_x else (-sn[d], cs[d])
        h = F32(0.5) * sigma
        hx, hy = h * ux, h * uy
        px, py = s[d, 0], s[d, 1]
        s[d, 2 if along_x else 3] = sigma
        s[t, 2:] = s[d, 2:]
        xmax, ymax = F32(W) - F32(1), F32(H) - F32(1)
        s[d, 0], s[d, 1] = clamp(px - hx, F32(0), xmax), clamp(py - hy, F32(0), ymax)
        s[t, 0], s[t, 1] = clamp(px + hx, F32(0), xmax), clamp(py + hy, F32(0), ymax)
        a[d] = 0
        a[t] = 0
        ids.append((d, t))
    return np.array(ids, dtype=np.int32).reshape(-1, 2), s, a


def random_case(rng, n, W, H):
    s = np.zeros((n, 9), dtype=F32)
    s[:, 0] = rng.uniform(0, W - 1, n)
    s[:, 1] = rng.uniform(0, H - 1, n)
    s[:, 2:4] = rng.choice([1.0, 1.2, 1.6, 3.0, 8.0, 40.0, 700.0, 1024.0], (n, 2))
    s[:, 4] = rng.uniform(-7, 7, n)
    s[:, 5:8] = rng.uniform(0, 1, (n, 3))
    s[:, 8] = rng.uniform(0.1, 1.0, n)
    a = rng.normal(size=(n, 18)).astype(F32)
    st = np.zeros((n, 3), dtype=F32)
    st[:, 0:2] = rng.choice([0.0, 0.0, 1e-3, 0.5, 0.5, 7.0], (n, 2)) * rng.choice([1.0, 1.0, 3.0], (n, 1))   # zeros and ties
    st[:, 2] = rng.choice([0.0, 0.0, 0.25, 0.25, 2.0, 30.0, 1e3], n)                                           # zeros and ties
    return st, s, a


def same(got, want):
    (gi, gs, ga), (wi, ws, wa) = got, want
    assert gi.tolist() == wi.tolist()
    assert gs.tobytes() == ws.tobytes() and ga.tobytes() == wa.tobytes()


@pytest.mark.parametrize("seed", range(24))
def test_planner_equals_the_numpy_restatement_on_random_inputs(seed, sincos):
    rng = np.random.default_rng(seed)
    n = int(rng.choice([2, 3, 17, 200, 1000]))
    W, H = int(rng.choice([1, 40, 268])), int(rng.choice([1, 17, 213]))
    st, s, a = random_case(rng, n, W, H)
    passes = int(rng.choice([1, 3, 10]))
    max_moves = int(rng.choice([1, 5, n // 3 + 1, n, n + 7]))
    min_weight = float(rng.choice([0.1, 0.25, 1.0, 50.0]))
    shrink = float(rng.choice([1.6, 1.0, 2.5, 0.5]))
    got = plan(st, passes, max_moves, min_weight, shrink, W, H, s, a)
    same(got, plan_numpy(st, passes, max_moves, min_weight, shrink, W, H, s, a, sincos))
    ids = got[0]
    if len(ids):
        assert len(set(ids.ravel().tolist())) == ids.size      # every changed row once: donors and starved are disjoint
        untouched = np.setdiff1d(np.arange(n), ids.ravel())
        assert got[1][untouched].tobytes() == s[untouched].tobytes() and got[2][untouched].tobytes() == a[untouched].tobytes()
        assert not got[2][ids.ravel()].any()                    # the moments of both rows are zero


def _edge_cases():
    """name -> (stats, passes, max_moves, min_weight, shrink, W, H, splats, adams, expected (donor, starved) pairs or None)."""
    rng = np.random.default_rng(99)
    out = {}
    # ties: w equal among 1, 2, 4 (starved, index order), a equal among 0, 3, 5 (donors, index order)
    st, s, a = random_case(rng, 6, 64, 48)
    st[:] = [[3, 4, 9], [0, 0, 0.5], [0, 0, 0.5], [5, 0, 9], [9, 9, 0.5], [0, 5, 9]]
    out["ties_by_index"] = (st, 1, 6, 1.0, 1.6, 64, 48, s, a, [(0, 1), (3, 2), (5, 4)])
    out["ties_max_moves_2"] = (st, 1, 2, 1.0, 1.6, 64, 48, s, a, [(0, 1), (3, 2)])
    out["max_moves_0"] = (st, 1, 0, 1.0, 1.6, 64, 48, s, a, [])
    out["max_moves_beyond_n"] = (st, 1, 1000, 1.0, 1.6, 64, 48, s, a, [(0, 1), (3, 2), (5, 4)])
    out["min_weight_0"] = (st, 1, 6, 0.0, 1.6, 64, 48, s, a, [])              # nothing is below 0
    out["min_weight_inf_all_starved"] = (st, 1, 6, INF, 1.6, 64, 48, s, a, [])  # every splat starved: no donor, no move
    out["passes_scale_the_threshold"] = (st, 20, 6, 1.0, 1.6, 64, 48, s, a, [])  # 9 / 20 < 1: all starved again
    # donors with a == 0 are skipped: only splat 2 can give
    st2 = np.array([[0, 0, 5], [0, 0, 0.1], [1e-30, 0, 5], [0, 0, 0.2]], dtype=F32)
    st3, s3, a3 = random_case(rng, 4, 64, 48)
    out["zero_gradient_donors_skipped"] = (st2, 1, 4, 1.0, 1.6, 64, 48, s3, a3, [(2, 1)])
    # clamps: a donor in the corner with a huge scale along x (position clamps both ways), a scale that shrinks below 1,
    # and a shrink < 1 that grows a scale past 1024
    s4 = np.zeros((6, 9), dtype=F32)
    s4[:, 5:9] = 0.5
    s4[0, :5] = [0.5, 47.0, 900.0, 3.0, 0.3]
    s4[1, :5] = [63.0, 0.0, 2.0, 800.0, 2.0]
    s4[2, :5] = [30.0, 20.0, 1.2, 1.1, -1.0]
    st4 = np.array([[9, 0, 5], [8, 0, 5], [7, 0, 5], [0, 0, 0], [0, 0, 0], [0, 0, 0]], dtype=F32)
    a4 = np.ones((6, 18), dtype=F32)
    out["position_and_scale_clamps"] = (st4, 1, 3, 1.0, 1.6, 64, 48, s4, a4, [(0, 3), (1, 4), (2, 5)])
    out["shrink_below_one_clamps_at_1024"] = (st4, 1, 3, 1.0, 0.5, 64, 48, s4, a4, [(0, 3), (1, 4), (2, 5)])
    z = np.zeros((0, 3), dtype=F32)
    out["n_0"] = (z, 1, 5, 1.0, 1.6, 64, 48, np.zeros((0, 9), dtype=F32), np.zeros((0, 18), dtype=F32), [])
    st1, s1, a1 = random_case(rng, 1, 64, 48)
    st1[:] = [[1, 1, 0]]
    out["n_1_starved_alone"] = (st1, 1, 5, 1.0, 1.6, 64, 48, s1, a1, [])
    st1b = st1.copy()
    st1b[:] = [[1, 1, 9]]
    out["n_1_donor_alone"] = (st1b, 1, 5, 1.0, 1.6, 64, 48, s1, a1, [])
    return out


EDGES = _edge_cases()


@pytest.mark.parametrize("name", sorted(EDGES))
def test_planner_edges(name, sincos):
    st, passes, max_moves, min_weight, shrink, W, H, s, a, pairs = EDGES[name]
    got = plan(st, passes, max_moves, min_weight, shrink, W, H, s, a)
    assert got[0].tolist() == [list(p) for p in pairs]
    same(got, plan_numpy(st, passes, max_moves, min_weight, shrink, W, H, s, a, sincos))
    if not pairs:
        assert got[1].tobytes() == s.tobytes() and got[2].tobytes() == a.tobytes()
    if name == "position_and_scale_clamps":
        g = got[1]
        assert g[0, 2] == F32(900.0) / F32(1.6) and g[0, 0] == 0.0 and g[3, 0] == 63.0    # both halves hit an image edge
        assert g[1, 3] == F32(500.0) and g[1, 1] == 47.0 and g[4, 1] == 0.0                # along sy: the y axis of the splat
        assert g[2, 2] == 1.0 and g[2, 3] == F32(1.1)                                      # 1.2 / 1.6 clamps to 1
        assert g[3, 2:].tobytes() == g[0, 2:].tobytes() and g[3, 0:2].tobytes() != g[0, 0:2].tobytes()
    if name == "shrink_below_one_clamps_at_1024":
        assert got[1][0, 2] == 1024.0 and got[1][1, 3] == 1024.0


def test_planner_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The stand-alone program, every array exactly as large as the contract says, on every edge input: same bytes as the
    shim, exit status 0, nothing on stderr."""
    exe = str(tmp_path / "s2d_density_main")
    subprocess.check_call(["g++", "-O1", "-g", "-ffp-contract=off", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(HC_DIR, "s2d_density_main.cpp"), "-lm"])
    for name in sorted(EDGES):
        st, passes, max_moves, min_weight, shrink, W, H, s, a, _ = EDGES[name]
        n = len(s)
        src, dst = str(tmp_path / (name + ".in")), str(tmp_path / (name + ".out"))
        with open(src, "wb") as f:
            f.write(struct.pack("<5i2f", n, passes, max_moves, W, H, min_weight, shrink))
            f.write(np.ascontiguousarray(st, dtype=F32).tobytes() + np.ascontiguousarray(s, dtype=F32).tobytes() +
                    np.ascontiguousarray(a, dtype=F32).tobytes())
        r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", (name, r.returncode, r.stderr[-2000:])
        ids, gs, ga = plan(st, passes, max_moves, min_weight, shrink, W, H, s, a)
        raw = open(dst, "rb").read()
        moves = struct.unpack_from("<i", raw)[0]
        assert moves == len(ids)
        want = ids.astype("<i4").tobytes() + gs.tobytes() + ga.tobytes()
        assert raw[4:] == want, name
