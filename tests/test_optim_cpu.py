"""CPU tests of the optimiser controls (include/splat2d.h, s2d_set_optim / s2d_optim_rates_at / s2d_set_frozen).

The composite oracle step of tests/optim_ref.py is what every GPU comparison of tests/test_gpu_optim.py rests on: here it is
held to the plain oracle step where the two must agree.  The host side of the feature -- validation and the rate formula,
csrc/s2d_optim_rates.h -- is compiled by g++ into a shim of its own (tests/hostcheck/s2d_optim_check.cpp) and held to the
header's words and to a float64 NumPy restatement.
"""
import ctypes as C
import importlib
import os
import subprocess
import tempfile

import numpy as np
import pytest

import adam_cases as A
import optim_hostcheck
import optim_ref as R
import oracle_lib as O

S2D = importlib.import_module("2dgaussiansplatting_amd")
F = np.float32
W0, H0 = 37, 21


def config(rate=R.TABLE_RATES, ratio=R.TABLE_RATIOS, T=R.TABLE_T):
    cfg = S2D._OptimConfig()
    cfg.struct_size = C.sizeof(S2D._OptimConfig)
    for g in range(5):
        cfg.rate[g], cfg.final_ratio[g] = rate[g], ratio[g]
    cfg.decay_iterations = T
    return cfg


def shim_rates(cfg, t, training_rate=0.05):
    out = np.zeros(5, dtype=F)
    optim_hostcheck.load().oc_rates_at(C.byref(cfg) if cfg is not None else None, training_rate, t, O._p(out))
    return out


# ---- the composite oracle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp32", [False, True])
@pytest.mark.parametrize("n", [1, 257, 777])
def test_composite_step_with_equal_rates_is_the_oracle_step(n, fp32):
    t = A.finite_table(n, W0, H0)
    plain = A.OracleState(t.splats, t.adams, W0, H0, fp32=fp32)
    comp = R.CompositeState(t.splats, t.adams, W0, H0, fp32=fp32)
    for s in range(t.grads.shape[0]):
        assert plain.step(t.grads[s], s % 2 == 1) == comp.step(t.grads[s], s % 2 == 1, np.full(5, A.LR, dtype=F)) == 0
        assert comp.splats.tobytes() == plain.splats.tobytes() and comp.adams.tobytes() == plain.adams.tobytes(), s
        assert comp.beta1t.tobytes() == plain.beta1t.tobytes() and comp.beta2t.tobytes() == plain.beta2t.tobytes()
        assert comp.iterations == plain.iterations


def test_composite_step_columns_and_frozen_rows():
    """Each group's columns are those of a plain step at that group's rate; frozen rows are the rows before the step."""
    n = 300
    t = A.finite_table(n, W0, H0, steps=1)
    rates = np.array(R.TABLE_RATES, dtype=F)
    frozen = np.arange(n) % 3 == 0
    comp = R.CompositeState(t.splats, t.adams, W0, H0)
    assert comp.step(t.grads[0], True, rates, frozen) == 0
    for g in range(5):
        one = R.CompositeState(t.splats, t.adams, W0, H0)
        one.step(t.grads[0], True, np.full(5, rates[g], dtype=F))
        cols = R.GROUP_COLUMNS[g]
        assert comp.splats[~frozen][:, cols].tobytes() == one.splats[~frozen][:, cols].tobytes(), g
        assert comp.adams[~frozen][:, cols].tobytes() == one.adams[~frozen][:, cols].tobytes(), g
    assert comp.splats[frozen].tobytes() == t.splats[frozen].tobytes() and comp.adams[frozen].tobytes() == t.adams[frozen].tobytes()


def test_composite_status_ignores_frozen_rows():
    t = A.nonfinite_table(2, "nan")
    rates = np.array(R.TABLE_RATES, dtype=F)
    assert R.CompositeState(t.splats, t.adams, t.W, t.H).step(t.grads[0], True, rates) == 1
    frozen = np.zeros(t.n, dtype=bool)
    frozen[A.NONFINITE_ROW] = True
    o = R.CompositeState(t.splats, t.adams, t.W, t.H)
    assert o.step(t.grads[0], True, rates, frozen) == 0
    assert o.splats[A.NONFINITE_ROW].tobytes() == t.splats[A.NONFINITE_ROW].tobytes()


def test_mini_trace_with_equal_rates_ends_where_the_reference_does():
    """The oracle loop of optim_ref with five times 0.05 is the reference's run: 5934.9042 ... 84.7616 after 300 iterations
    (the squirrel mini, 1024 splats), the plain figure of DESIGN.md section 15's table."""
    tgt = O.target_rgba32f(O.load_s2di(os.path.join(O.GOLDEN, "squirrel_cls_mini_268x213.s2di")))
    _, trace = R.oracle_loop(tgt, 1024, 300, lambda t: np.full(5, A.LR, dtype=F))
    assert "%.4f" % trace[0] == "5934.9042" and "%.4f" % trace[299] == "84.7616", (trace[0], trace[299])


# ---- the struct --------------------------------------------------------------------------------------------------------
def test_optim_config_layout_matches_header():
    code = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "splat2d.h"
    int main(void) {
        printf("%zu %zu %zu %zu\n", sizeof(s2d_optim_config), offsetof(s2d_optim_config, rate),
               offsetof(s2d_optim_config, final_ratio), offsetof(s2d_optim_config, decay_iterations));
        return 0;
    }'''
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write(code)
        subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(O.ROOT, "include"), src, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    B = S2D._OptimConfig
    assert got == [C.sizeof(B), B.rate.offset, B.final_ratio.offset, B.decay_iterations.offset] == [48, 4, 24, 44]
    assert optim_hostcheck.load().oc_config_size() == 48
    assert [optim_hostcheck.load().oc_group_of(k) for k in range(9)] == list(R.GROUP_OF)
    assert S2D.OPTIM_GROUPS == ("pos", "scale", "rot", "color", "opacity")


# ---- the rate formula --------------------------------------------------------------------------------------------------
def test_rate_is_exact_without_decay():
    rate = (0.5, 0.2, 0.1, 0.05, 0.3)
    want = np.array(rate, dtype=F)
    for ratio, T in (((0.1, 0.5, 0.3, 0.2, 0.25), 0), ((1, 1, 1, 1, 1), 7), ((0, 0, 0, 0, 0), 7)):
        for t in (0, 1, 3, 7, 8, 1000, 2 ** 31 - 1):
            assert shim_rates(config(rate, ratio, T), t).tobytes() == want.tobytes(), (ratio, T, t)
    # ratio 1 for some groups only: those stay exact while the others decay
    got = shim_rates(config(rate, (0.1, 1, 0, 0.5, 1), 10), 5)
    assert got[1] == want[1] and got[2] == want[2] and got[4] == want[4] and got[0] < want[0] and got[3] < want[3]
    assert shim_rates(None, 5, 0.07).tobytes() == np.full(5, 0.07, dtype=F).tobytes()


@pytest.mark.parametrize("T", [1, 4, 300, 30000])
def test_rate_formula_against_float64_restatement(T):
    rate, ratio = (0.5, 0.2, 0.1, 0.05, 1e-3), (0.1, 0.5, 1.0, 3.0, 1e-4)
    cfg = config(rate, ratio, T)
    ts = sorted(set([0, 1, 2, 3, T // 2, T - 1, T, T + 1, 2 * T, 2 ** 31 - 1]))
    prev = None
    for t in ts:
        got, want = shim_rates(cfg, t), R.rates_f64(rate, ratio, T, t)
        assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= O.ulp32(want)).all(), (t, got, want)  # 1 ulp (fp32)
        assert got[2] == F(rate[2])                                  # ratio 1: exact
        if t >= T:
            assert got.tobytes() == shim_rates(cfg, T).tobytes(), t  # constant from T on
        if prev is not None:                                         # monotone: down for ratio < 1, up for ratio > 1
            assert (got[[0, 1, 4]] <= prev[[0, 1, 4]]).all() and got[3] >= prev[3], t
        prev = got
    end = shim_rates(cfg, T)
    assert (np.abs(end.astype(np.float64) - (np.array(rate, F) * np.array(ratio, F)).astype(np.float64)) <= O.ulp32(end)).all()
    assert shim_rates(cfg, 0).tobytes() == np.array(rate, dtype=F).tobytes()   # pow(x, 0) == 1


def test_rate_is_monotone_step_by_step():
    cfg = config((0.5, 0.2, 0.1, 0.05, 0.05), (0.1, 0.5, 1, 2.0, 0.25), 300)
    r = np.stack([shim_rates(cfg, t) for t in range(0, 320)])
    assert (np.diff(r[:301, 0]) < 0).all() and (np.diff(r[:301, 1]) < 0).all() and (np.diff(r[:301, 3]) > 0).all()
    assert (np.diff(r[:, 2]) == 0).all() and (np.diff(r[300:], axis=0) == 0).all()


# ---- refusals ----------------------------------------------------------------------------------------------------------
BAD = [("struct_size", lambda c: setattr(c, "struct_size", 44)),
       ("rate 0", lambda c: c.rate.__setitem__(0, 0.0)),
       ("rate < 0", lambda c: c.rate.__setitem__(3, -0.05)),
       ("rate inf", lambda c: c.rate.__setitem__(1, float("inf"))),
       ("rate nan", lambda c: c.rate.__setitem__(4, float("nan"))),
       ("ratio < 0", lambda c: c.final_ratio.__setitem__(2, -0.5)),
       ("ratio inf", lambda c: c.final_ratio.__setitem__(0, float("inf"))),
       ("ratio nan", lambda c: c.final_ratio.__setitem__(4, float("nan"))),
       ("T < 0", lambda c: setattr(c, "decay_iterations", -1))]


def test_validation_refuses_what_the_header_lists():
    L = optim_hostcheck.load()
    assert L.oc_refused(C.byref(config())) == 0
    assert L.oc_refused(C.byref(config(ratio=(0, 0, 0, 0, 0), T=0))) == 0     # ratio 0 means 1
    assert L.oc_refused(C.byref(config(ratio=(5.0, 0.5, 1, 1, 1), T=2 ** 31 - 1))) == 0
    assert L.oc_refused(None) == 1
    for name, spoil in BAD:
        cfg = config()
        spoil(cfg)
        assert L.oc_refused(C.byref(cfg)) == 1, name
    cfg = config(T=0)     # T == 0: the ratios are still validated
    cfg.final_ratio[1] = -1.0
    assert L.oc_refused(C.byref(cfg)) == 1


def test_entry_points_reject_a_null_context():
    S2D._build.build_hip_library()
    L = S2D.load_library()
    out = (C.c_float * 5)()
    assert L.s2d_set_optim(None, C.byref(config())) == 1 and L.s2d_optim_rates_at(None, 0, out) == 1
    assert L.s2d_set_frozen(None, None) == 1 and L.s2d_set_frozen_device(None, None) == 1
