"""CPU tests of the alive set (include/splat2d.h, "the alive set"): the header and the binding name
the new calls, the NumPy restatements of tests/alive_ref.py on hand-written cases, the planners of s2d_relocate / s2d_reseed
under NaN-masked statistics (the g++ shims of test_density_plan_cpu.py and test_seed_cpu.py, imported), and what the entry
points and the host tool refuse before they touch a device."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import alive_ref as AR
import oracle_lib as O
import seed_ref as SR
import test_density_plan_cpu as DP
import test_seed_cpu as SC

S2D = importlib.import_module("2dgaussiansplatting_amd")
HEADER = os.path.join(O.ROOT, "include", "splat2d.h")
NEW_NAMES = ["s2d_set_alive", "s2d_set_alive_device", "s2d_get_alive", "s2d_prune_config", "s2d_prune", "s2d_grow"]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_header_and_binding_name_the_alive_calls():
    text = open(HEADER).read()
    for name in NEW_NAMES:
        assert re.search(r"\b%s\b" % name, text), name
    for name in NEW_NAMES:
        if name != "s2d_prune_config":
            assert re.search(r"^int %s\(s2d_ctx\* ctx" % name, text, flags=re.M), name
            assert name in S2D.ABI_SYMBOLS
    assert re.search(r"#define S2D_ABI_VERSION 2\b", text)                      # new entry points alone do not bump it
    for method in ("set_alive", "set_alive_device", "alive", "prune", "grow"):
        assert callable(getattr(S2D.Trainer, method)), method
    op_src = open(os.path.join(O.ROOT, "2dgaussiansplatting_amd", "torch_op.py")).read()
    assert "def set_alive(self, mask)" in op_src


def test_prune_config_layout_matches_header():
    text = open(HEADER).read()
    body = re.search(r"typedef struct s2d_prune_config \{(.*?)\} s2d_prune_config;", text, flags=re.S).group(1)
    fields = re.findall(r"^\s*(uint32_t|float)\s+(\w+);", body, flags=re.M)
    assert fields == [("uint32_t", "struct_size"), ("float", "min_weight"), ("float", "min_opacity")]
    assert [f[0] for f in S2D._PruneConfig._fields_] == [f[1] for f in fields] and C.sizeof(S2D._PruneConfig) == 12


def test_prune_rule_on_hand_written_cases():
    alive = np.array([1, 1, 1, 1, 0, 1, 1], dtype=bool)
    stats = np.zeros((7, 3), dtype=np.float32)
    stats[:, 2] = [0.0, 2.9999, 3.0, 30.0, 0.0, np.nan, 1.5]
    opacity = np.array([0.9, 0.2, 0.5, 0.49999, 0.1, 0.1, np.nan], dtype=np.float32)
    # weight per pass (3 passes) below 1: rows 0 and 1 (2.9999 / 3 < 1), not row 2 (exactly 1), not the NaN, not the dead row
    assert AR.prune(alive, stats, 3, opacity, min_weight=1.0).tolist() == [False, False, True, True, False, True, False]
    # opacity below 0.5: rows 1, 3 and 5; a NaN opacity prunes nothing; row 4 was dead and stays dead
    assert AR.prune(alive, stats, 3, opacity, min_opacity=0.5).tolist() == [True, False, True, False, False, False, True]
    # both: the union
    assert AR.prune(alive, stats, 3, opacity, 1.0, 0.5).tolist() == [False, False, True, False, False, False, False]
    # a criterion that is off does not look at its input
    assert AR.prune(alive, None, 0, opacity, 0.0, 0.05).tolist() == alive.tolist()
    # the threshold is the float32 the ABI carries, the quotient a double: 1/3 rounded to float32 is above 1/3
    third = np.zeros((1, 3), dtype=np.float32)
    third[0, 2] = 1.0
    assert AR.prune([True], third, 3, [1.0], min_weight=np.float32(1.0) / np.float32(3.0)).tolist() == [False]


def test_lowest_dead_and_compaction_on_hand_written_cases():
    alive = np.array([0, 1, 0, 0, 1, 0], dtype=bool)
    assert AR.lowest_dead(alive, 2).tolist() == [0, 2]
    assert AR.lowest_dead(alive, 10 ** 6).tolist() == [0, 2, 3, 5]
    assert AR.lowest_dead(alive, 0).tolist() == [] and AR.lowest_dead(np.ones(4, dtype=bool), 3).tolist() == []
    rows = np.arange(12, dtype=np.float32).reshape(6, 2)
    c = AR.compact(rows, alive)
    assert c.tolist() == [[2, 3], [8, 9]] and c.flags["C_CONTIGUOUS"]
    back = AR.expand(c * 10, alive, rows)
    assert back[1].tolist() == [20, 30] and back[4].tolist() == [80, 90] and back[[0, 2, 3, 5]].tolist() == rows[[0, 2, 3, 5]].tolist()
    m = AR.nan_masked(np.ones((6, 3), dtype=np.float32), alive)
    assert np.isnan(m[~alive]).all() and (m[alive] == 1).all()
    for n in (1, 255, 256, 257, 777):
        ms = AR.masks(n)
        assert ms["all"].all() and not ms["none"].any() and ms["one"].sum() == 1 and ms["every_second"].sum() == (n + 1) // 2
        assert ("first_block_dead" in ms) == (n > 256) and ("last_20" in ms) == (n > 20)
        if n > 256:
            assert not ms["first_block_dead"][:256].any() and ms["first_block_dead"][256:].all()
        if n > 20:
            assert ms["last_20"].sum() == 20 and ms["last_20"][-20:].all()
        assert all(v.shape == (n,) and v.dtype == bool for v in ms.values())


@pytest.mark.parametrize("seed", range(6))
def test_planners_never_name_a_dead_row_under_nan_masked_statistics(seed):
    """s2d_relocate and s2d_reseed hand the planners the statistics with NaN in the dead rows: neither the relocation planner
    (donors and starved rows) nor the starved selection may then name one -- with thresholds under which, unmasked, they do."""
    rng = np.random.default_rng(4000 + seed)
    n, W, H = int(rng.choice([1, 40, 257, 777])), 96, 80
    stats = rng.uniform(0, 4, (n, 3)).astype(np.float32)
    stats[rng.random(n) < 0.3, 2] = 0.0                                        # plenty of starved rows
    splats = np.zeros((n, 9), dtype=np.float32)
    splats[:, 0], splats[:, 1] = rng.uniform(0, W - 1, n), rng.uniform(0, H - 1, n)
    splats[:, 2], splats[:, 3] = rng.uniform(1, 6, n), rng.uniform(1, 6, n)
    splats[:, 4], splats[:, 5:8], splats[:, 8] = rng.uniform(-3, 3, n), rng.uniform(0, 1, (n, 3)), rng.uniform(0.1, 1, n)
    adams = rng.uniform(-1, 1, (n, 18)).astype(np.float32)
    passes = 3
    for name, alive in AR.masks(n, seed).items():
        masked = AR.nan_masked(stats, alive)
        dead = set(np.nonzero(~alive)[0].tolist())
        for mw in (float("inf"), 0.5, float(np.median(stats[:, 2]) / passes) + 1e-3):
            ids, s_after, a_after = DP.plan(masked, passes, n, mw, 1.6, W, H, splats, adams)
            assert not (set(ids.ravel().tolist()) & dead), (name, mw)
            untouched = np.setdiff1d(np.arange(n), ids.ravel())
            assert s_after[untouched].tobytes() == splats[untouched].tobytes() and a_after[untouched].tobytes() == adams[untouched].tobytes()
            starved = SC.shim_starved(masked, passes, n, mw)
            assert not (set(starved.tolist()) & dead), (name, mw)
            assert starved.tolist() == SR.starved(masked, passes, n, mw).tolist()
            # the premise: unmasked, the same call does name rows that are dead under this mask (where there are any to name)
            if name in ("every_second", "random_half") and n >= 40 and mw != float("inf"):
                assert set(SC.shim_starved(stats, passes, n, mw).tolist()) & dead, (name, mw)


def _half_created_context(L, reference_order=False):
    c = S2D._Config()
    c.struct_size = C.sizeof(S2D._Config)
    c.width, c.height, c.n_splats = 32, 16, 8
    c.flags = S2D.S2D_CFG_REFERENCE_ORDER if reference_order else 0
    h = C.c_void_p()
    rc = L.s2d_create(C.byref(c), C.byref(h))
    assert rc in (0, 2) and h.value
    return h


def test_entry_points_check_arguments_without_a_device():
    S2D._build.build_hip_library()
    L = S2D.load_library()
    good = S2D._PruneConfig(C.sizeof(S2D._PruneConfig), 0.0, 0.5)
    seed = SC.good_config()
    count = C.c_int32(-7)
    mask = np.ones(8, dtype=np.uint8)
    assert L.s2d_set_alive(None, _p(mask)) == 1 and L.s2d_set_alive_device(None, None) == 1
    assert L.s2d_get_alive(None, _p(mask), C.byref(count)) == 1
    assert L.s2d_prune(None, C.byref(good), C.byref(count)) == 1 and L.s2d_grow(None, C.byref(seed), None, 1, C.byref(count)) == 1
    h = _half_created_context(L)
    try:
        assert L.s2d_prune(h, None, C.byref(count)) == 1 and count.value == 0
        for what, cfg in (("struct_size", S2D._PruneConfig(8, 0.0, 0.5)), ("both off", S2D._PruneConfig(12, 0.0, 0.0)),
                          ("negative weight", S2D._PruneConfig(12, -1.0, 0.5)), ("negative opacity", S2D._PruneConfig(12, 1.0, -0.5)),
                          ("NaN weight", S2D._PruneConfig(12, float("nan"), 0.5)), ("NaN opacity", S2D._PruneConfig(12, 0.5, float("nan")))):
            assert L.s2d_prune(h, C.byref(cfg), C.byref(count)) == 1, what
            assert L.s2d_last_error(h)
        assert L.s2d_prune(h, C.byref(S2D._PruneConfig(12, 1.0, 0.0)), C.byref(count)) == 5      # no statistics pass yet
        assert L.s2d_grow(h, None, None, 1, C.byref(count)) == 1
        assert L.s2d_grow(h, C.byref(seed), None, -1, C.byref(count)) == 1
        for what, change in SC.bad_configs():
            cfg = SC.good_config()
            for k, v in change.items():
                setattr(cfg, k, v)
            assert L.s2d_grow(h, C.byref(cfg), None, 1, C.byref(count)) == 1, what
        ids = np.array([0, 1], dtype=np.int32)                                  # without a set every row is alive
        assert L.s2d_grow(h, C.byref(seed), _p(ids), 2, C.byref(count)) == 1 and count.value == 0
        assert L.s2d_grow(h, C.byref(seed), None, 1, C.byref(count)) == 5       # the arguments are fine: no target yet
    finally:
        L.s2d_destroy(h)
    h = _half_created_context(L, reference_order=True)
    try:
        assert L.s2d_set_alive(h, _p(mask)) == 1 and L.s2d_set_alive(h, None) == 1 and L.s2d_set_alive_device(h, None) == 1
        assert L.s2d_get_alive(h, _p(mask), C.byref(count)) == 1
        assert L.s2d_prune(h, C.byref(good), C.byref(count)) == 1 and L.s2d_grow(h, C.byref(seed), None, 1, C.byref(count)) == 1
        assert b"REFERENCE_ORDER" in L.s2d_last_error(h)
    finally:
        L.s2d_destroy(h)


def test_host_tool_refuses_what_it_cannot_combine():
    """The alive options with --gpus > 1, --reference-order or a checkpoint, --prune-every beside another owner of the
    statistics window, and values out of range: refused with a message before any device is touched."""
    S2D._build.build_hip_library()
    exe = S2D._build.build_host_program()
    base = [exe, "--synthetic", "64x48", "--splats", "50", "--iters", "4"]
    cases = ((["--alive-from", "10", "--gpus", "2"], "one context"), (["--grow-every", "2", "--grow-count", "5", "--gpus", "2"], "one context"),
             (["--prune-every", "2", "--gpus", "2"], "one context"), (["--alive-from", "10", "--reference-order"], "--reference-order"),
             (["--alive-from", "10", "--save-checkpoint", "x.ckpt"], "checkpoint"), (["--prune-every", "2", "--load-checkpoint", "x.ckpt"], "checkpoint"),
             (["--prune-every", "2", "--relocate-every", "2"], "statistics window"), (["--prune-every", "2", "--reseed-every", "2"], "statistics window"),
             (["--grow-every", "2"], "go together"), (["--grow-count", "2"], "go together"),
             (["--alive-from", "51"], "usage"), (["--alive-from", "-1"], "usage"), (["--prune-every", "2", "--prune-window", "0"], "usage"),
             (["--prune-every", "2", "--prune-min-weight", "0"], "usage"), (["--grow-every", "2", "--grow-count", "5", "--grow-scale", "-1"], "usage"))
    for extra, word in cases:
        r = subprocess.run(base + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
        assert r.returncode == 2 and word in r.stderr and not r.stdout, (extra, r.returncode, r.stderr[:200])
    usage = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True).stderr
    assert "--alive-from" in usage and "does not carry the set" in usage and "provisional" in usage
