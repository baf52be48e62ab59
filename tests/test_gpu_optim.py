"""The optimiser controls on the GPU (include/splat2d.h, "optimiser controls"; adam_controls_kernel,
csrc/s2d_optim_controls.hip): rates per parameter group with their decay, and frozen splats.

Expected values always come from the COMPOSITE oracle of tests/optim_ref.py (one s2do_adam_step per distinct rate, columns
merged by group, frozen rows restored), fed with the library's own rounded rates, Trainer.rates_at(), so no comparison depends
on whose pow() rounds how.  Gradients are injected as tests/test_gpu_adam_step.py does, and the comparison is that file's
same_state: parameters, moments, beta words and the iteration count with identical bits (adam_cases.assert_same_bits), and
an all-+0 gradient buffer after every step.  tests/test_optim_cpu.py asserts what these tests assume about the composite
oracle and about the rate formula.
"""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import adam_cases as A
import optim_ref as R
import oracle_lib as O
import test_gpu_adam_step as T

pytestmark = pytest.mark.gpu

S2D = importlib.import_module("2dgaussiansplatting_amd")
F = np.float32
W0, H0 = T.W0, T.H0
MINI = os.path.join(O.GOLDEN, "squirrel_cls_mini_268x213.s2di")
S2D_E_INVALID, S2D_E_NONFINITE = 1, 3


def table_config(t):
    """The decaying configuration of the table tests: the rate changes every step until T = 4, then stands."""
    r, q = R.TABLE_RATES, R.TABLE_RATIOS
    t.set_optim(pos=r[0], scale=r[1], rot=r[2], color=r[3], opacity=r[4], final_ratio=q, decay_iterations=R.TABLE_T)


def run_table(r, t, o, what, frozen=None, flags=None):
    """T.run_table under the controls: the oracle's step is the composite one at rates_at(iteration)."""
    for s in range(t.grads.shape[0]):
        flag = (s % 2 == 1) if flags is None else flags[s]
        rates = r.t.rates_at(o.iterations)
        assert o.step(t.grads[s], flag, rates, frozen) == 0
        r.step(t.grads[s], flag)
        r.t.synchronize()
        T.same_state(r, o, "%s, step %d" % (what, s))


def mini_target():
    return O.target_rgba32f(O.load_s2di(MINI))


# ---------------------------------------------------------------------------------------------------------------------
# 1, 2: the tables of the plain launch, through the second instantiation with a rate that changes every step
# ---------------------------------------------------------------------------------------------------------------------
def test_rates_at_follows_the_header():
    with T.rig(W0, H0, 3, bind=False, training_rate=0.07) as r:
        assert r.t.rates_at(0).tobytes() == np.full(5, 0.07, dtype=F).tobytes()     # no configuration: training_rate
        r.t.set_optim(pos=0.5)                                                       # omitted rates: training_rate
        assert r.t.rates_at(9).tobytes() == np.array([0.5, 0.07, 0.07, 0.07, 0.07], dtype=F).tobytes()
        table_config(r.t)
        for it in (0, 1, 2, 3, 4, 5, 1000):
            got, want = r.t.rates_at(it), R.rates_f64(R.TABLE_RATES, R.TABLE_RATIOS, R.TABLE_T, it)
            assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= O.ulp32(want)).all(), (it, got, want)
            assert got[2] == F(0.1) and got[3] == F(0.05)                            # ratio 1: exact
        assert r.t.rates_at(4).tobytes() == r.t.rates_at(77).tobytes() != r.t.rates_at(3).tobytes()
        r.t.set_optim(None)
        assert r.t.rates_at(3).tobytes() == np.full(5, 0.07, dtype=F).tobytes()


@pytest.mark.parametrize("fp32", [False, True])
@pytest.mark.parametrize("n", [1, 3, 255, 256, 257, 777])
def test_finite_tables_under_decaying_group_rates(n, fp32):
    for W, H in ((37, 21), (16, 16)):
        t = A.finite_table(n, W, H)
        o = R.CompositeState(t.splats, t.adams, W, H, fp32=fp32)
        with T.rig(W, H, n, adam_fp32=fp32) as r:
            table_config(r.t)
            r.load(o)
            run_table(r, t, o, "%dx%d n=%d fp32=%s" % (W, H, n, fp32))
            assert len({r.t.rates_at(s).tobytes() for s in range(6)}) == 5      # (a new rate in steps 0..4, then it stands)


@pytest.mark.parametrize("layout", A.DORMANT_LAYOUTS)
def test_dormant_tables_under_the_controls(layout):
    """The inert-block skip and both wake-ups in the second instantiation (adam_cases.dormant_table)."""
    t = A.dormant_table(layout)
    o = R.CompositeState(t.splats, t.adams, t.W, t.H)
    with T.rig(t.W, t.H, t.n) as r:
        table_config(r.t)
        r.load(o)
        run_table(r, t, o, "dormant layout %d" % layout)


# ---------------------------------------------------------------------------------------------------------------------
# 3: the finite guard
# ---------------------------------------------------------------------------------------------------------------------
def guard_case(r, t, flag, what, frozen_rows=None, start=2):
    """One step from iteration `start` (inside the decay): S2D_E_NONFINITE exactly where the composite oracle returns 1."""
    o = R.CompositeState(t.splats, t.adams, t.W, t.H, *A.beta_powers(start), start)
    r.load(o)
    frozen = None
    if frozen_rows is not None:
        frozen = np.zeros(t.n, dtype=bool)
        frozen[list(frozen_rows)] = True
    r.t.set_frozen(frozen)
    status = o.step(t.grads[0], flag, r.t.rates_at(start), frozen)
    r.step(t.grads[0], flag)
    if status:
        with pytest.raises(S2D.S2DError) as e:
            r.t.synchronize()
        assert e.value.code == S2D_E_NONFINITE, what
        assert r.t.stats()["first_nonfinite_iteration"] == start, what
    else:
        r.t.synchronize()
        assert r.t.stats()["first_nonfinite_iteration"] == -1, what
    T.same_state(r, o, what)
    return status, o


def test_finite_guard_nonfinite_gradients_and_frozen_offenders():
    with T.rig(W0, H0, 300) as r:
        table_config(r.t)
        for field, name in A.NONFINITE_CASES:
            t = A.nonfinite_table(field, name)
            what = "%s gradient %s" % (A.FIELDS[field], name)
            status, o = guard_case(r, t, True, what)
            assert status == A.nonfinite_status(field) and np.isnan(o.splats[A.NONFINITE_ROW, field]), what
            status, o = guard_case(r, t, True, what + ", row frozen", frozen_rows=[A.NONFINITE_ROW])
            assert status == 0 and o.splats[A.NONFINITE_ROW].tobytes() == t.splats[A.NONFINITE_ROW].tobytes(), what
            assert o.adams[A.NONFINITE_ROW].tobytes() == t.adams[A.NONFINITE_ROW].tobytes(), what


def test_finite_guard_overflow_table_and_frozen_offenders():
    with T.rig(W0, H0, 300) as r:
        table_config(r.t)
        for name, fields, want in A.OVERFLOW_CASES:
            t = A.overflow_table(fields)
            status, _ = guard_case(r, t, True, "overflow, " + name)
            assert status == want, name
            status, o = guard_case(r, t, True, "overflow, %s, rows frozen" % name, frozen_rows=A.OVERFLOW_ROWS)
            rows = list(A.OVERFLOW_ROWS)
            assert status == 0 and o.splats[rows].tobytes() == t.splats[rows].tobytes(), name


# ---------------------------------------------------------------------------------------------------------------------
# 4: frozen masks
# ---------------------------------------------------------------------------------------------------------------------
FROZEN_N = 773


def frozen_mask(name):
    m = np.zeros(FROZEN_N, dtype=bool)
    if name == "block":
        m[256:512] = True           # one whole block of the launch
    elif name == "every second":
        m[1::2] = True              # a frozen and a live record share 16-byte lines of the 9- and 18-word arrays
    else:
        m[:] = np.random.default_rng(30).random(FROZEN_N) < 0.3
    return m


@pytest.mark.parametrize("how", ["host", "device", "host, no rates"])
@pytest.mark.parametrize("mask_name", ["block", "every second", "random 30 %"])
def test_frozen_rows_stay_byte_identical(mask_name, how):
    mask = frozen_mask(mask_name)
    t = A.finite_table(FROZEN_N, W0, H0, steps=6)
    assert A.bits(t.grads[:5, 256:512]).any(axis=(1, 2)).all()     # (real gradients inside the frozen block, every step)
    o = R.CompositeState(t.splats, t.adams, W0, H0)
    with T.rig(W0, H0, FROZEN_N) as r:
        if how != "host, no rates":
            table_config(r.t)
        r.load(o)
        if how == "device":
            dmask = r.dev(mask.astype(np.uint8))
            r.t.set_frozen_device(dmask.data_ptr())
        else:
            r.t.set_frozen(mask)
        for s in range(5):
            assert o.step(t.grads[s], s % 2 == 1, r.t.rates_at(o.iterations), mask) == 0
            r.step(t.grads[s], s % 2 == 1)
            r.t.synchronize()
            what = "mask %s (%s), step %d" % (mask_name, how, s)
            T.same_state(r, o, what)       # (with it: every gradient +0, the frozen rows' included)
            sp, ad = r.state()[:2]
            assert sp[mask].tobytes() == t.splats[mask].tobytes() and ad[mask].tobytes() == t.adams[mask].tobytes(), what
        r.t.set_frozen(None) if how != "device" else r.t.set_frozen_device(0)
        assert o.step(t.grads[5], True, r.t.rates_at(o.iterations)) == 0      # clearing the mask resumes ordinary steps
        r.step(t.grads[5], True)
        r.t.synchronize()
        T.same_state(r, o, "mask %s cleared" % mask_name)
        assert (r.state()[0][mask] != t.splats[mask]).any()


def test_frozen_rows_rewritten_before_a_fused_step_are_projected():
    """With re-usable lists the step also projects what it wrote.  Rows written with s2d_rows_scatter leave the projection
    records stale; a frozen one among them is not updated by the step that follows but must still be projected: the next
    forward() is the oracle's forward of the same parameters."""
    W, H, n = 96, 80, 300
    tgt = O.synthetic_target(W, H)
    ot = O.OracleTrainer(tgt, n)
    t = A.finite_table(n, W, H, steps=1, seed=5)
    t.adams[:, 4], t.grads[:, :, 4] = 0.0, 0.0          # rot is not clamped: keep it where sin / cos are bitwise
    start = ot.splats.view(F).reshape(n, 9).copy()
    o = R.CompositeState(start, t.adams, W, H)
    mask = np.arange(n) % 2 == 1
    rows = np.array([7, 8, 150, 151], dtype=np.int32)     # two frozen, two live
    new = start[rows].copy()
    new[:, 0], new[:, 1], new[:, 2] = [5.0, 60.0, 90.0, 30.0], [70.0, 10.0, 40.0, 20.0], 6.0
    with T.rig(W, H, n, rebin_interval=8) as r:
        r.t.set_target_synthetic()
        table_config(r.t)
        r.load(o)
        r.t.set_frozen(mask)
        r.t.forward()
        ids, vals = r.dev(rows), r.dev(new)
        r.t.rows_scatter(S2D.ROWS_SPLATS, ids.data_ptr(), len(rows), vals.data_ptr())
        o.splats[rows] = new
        assert o.step(t.grads[0], False, r.t.rates_at(0), mask) == 0
        r.step(t.grads[0], False)
        r.t.forward()
        r.t.synchronize()
        T.same_state(r, o, "frozen rows rewritten")
        ot.splats[:] = o.splats.view(O.SPLAT_DTYPE).reshape(-1)
        assert r.t.get_image().tobytes() == ot.forward().tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# 5: a configuration that equals the defaults is another kernel with the same bytes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", [False, True])
def test_equal_rates_give_the_plain_launch_bytes(loss):
    tgt, n = mini_target(), 1024
    out = []
    for controls in (False, True):
        with S2D.Trainer(268, 213, n, deterministic=True) as t:
            t.set_target(tgt)
            t.init()
            if controls:
                t.set_optim(pos=0.05, scale=0.05, rot=0.05, color=0.05, opacity=0.05)
            mse = t.step_loss(5, 1.0, 0.0, 0.0)[1] if loss else t.step(5)
            ad = t.get_adam()
            t.forward()
            out.append((t.get_image().tobytes(), t.get_splats().tobytes(), ad[0].tobytes(), ad[1:], mse.tobytes()))
    assert out[0] == out[1]


# ---------------------------------------------------------------------------------------------------------------------
# 6: end to end in reference order
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["33x17", "mini"])
def test_reference_order_training_equals_the_oracle_loop(scene):
    if scene == "mini":
        tgt, n, iters, frozen, opacity = mini_target(), 1024, 10, None, False
    else:
        tgt, n, iters, frozen, opacity = O.synthetic_target(33, 17), 200, 30, np.arange(200) % 2 == 1, True
    H, W = tgt.shape[:2]
    with S2D.Trainer(W, H, n, reference_order=True) as t:
        t.set_target(tgt)
        t.init()
        table_config(t)
        t.set_frozen(frozen)
        t.optimize_opacity = opacity
        o, trace = R.oracle_loop(tgt, n, iters, t.rates_at, frozen, opacity)
        mse = t.step(iters)
        assert mse.tobytes() == np.array(trace, dtype=np.float64).tobytes(), (mse[-3:], trace[-3:])
        sp = t.get_splats()
        ad, b1, b2, it = t.get_adam()
        A.assert_same_bits(sp.view(F), o.splats.view(F), scene + ": parameters")
        A.assert_same_bits(ad.view(F), o.adams.view(F), scene + ": moments")
        assert (A.bits(b1), A.bits(b2), it) == (A.bits(o.beta1t[0]), A.bits(o.beta2t[0]), iters)
        if frozen is not None:
            first = O.OracleTrainer(tgt, n)
            assert sp[frozen].tobytes() == first.splats[frozen].tobytes() and (sp[~frozen] != first.splats[~frozen]).any()
        t.forward()
        image = t.get_image().tobytes()
    with S2D.Trainer(W, H, n, reference_order=True) as fresh:
        fresh.set_target(tgt)
        fresh.set_splats(sp)
        fresh.forward()
        assert fresh.get_image().tobytes() == image


# ---------------------------------------------------------------------------------------------------------------------
# 7: resume; what init() clears
# ---------------------------------------------------------------------------------------------------------------------
def test_resume_follows_the_schedule_and_init_clears_the_mask_only():
    n, k = 257, 3
    t = A.finite_table(n, W0, H0, steps=2)
    o = R.CompositeState(t.splats, t.adams, W0, H0, *A.beta_powers(k), k)
    with T.rig(W0, H0, n) as r:
        table_config(r.t)
        at = [r.t.rates_at(i).copy() for i in range(6)]
        r.load(o)                                          # set_adam(..., iterations = k)
        assert r.t.rates_at(k).tobytes() == at[k].tobytes() != at[0].tobytes()
        for s in range(2):                                 # the steps at k and k + 1 use the rates of k and k + 1
            assert o.step(t.grads[s], True, at[k + s]) == 0
            r.step(t.grads[s], True)
            r.t.synchronize()
            T.same_state(r, o, "resumed at %d, step %d" % (k, s))
        # init(): the mask goes, the rates stay (include/splat2d.h)
        r.t.set_frozen(np.ones(n, dtype=bool))
        r.t.init()
        assert r.t.rates_at(2).tobytes() == at[2].tobytes()
        first = r.t.get_splats().view(F).reshape(n, 9).copy()
        fresh = R.CompositeState(first, np.zeros((n, 9, 2), dtype=F), W0, H0)
        assert fresh.step(t.grads[0], True, at[0]) == 0
        r.step(t.grads[0], True)
        r.t.synchronize()
        T.same_state(r, fresh, "after init()")
        assert (fresh.splats != first).any()
        # set_splats keeps the mask
        r.t.set_frozen(np.ones(n, dtype=bool))
        r.t.set_splats(first.view(S2D.SPLAT_DTYPE).reshape(-1))
        r.step(t.grads[1], True)
        r.t.synchronize()
        assert r.state()[0].tobytes() == first.tobytes() and not A.bits(r.grads()).any()


# ---------------------------------------------------------------------------------------------------------------------
# 8: the gain
# ---------------------------------------------------------------------------------------------------------------------
# tools/optim_oracle_schedule.py: the composite oracle, 300 iterations of the mini, plain against R.GAIN_RATES
ORACLE_PLAIN, ORACLE_GROUPS = 84.7616, 68.6788
GAIN_BAR = 1.0 - 0.5 * (1.0 - ORACLE_GROUPS / ORACLE_PLAIN)   # half the oracle's relative gain (the rule of DESIGN.md section 14)


def test_group_rates_lower_the_final_error():
    """Deterministic, opacity off.  Half the oracle's gain leaves room for the different summation order of the two
    trajectories.
    Measured on an MI355X: plain 84.7402, group rates 68.1676, ratio 0.8044 (bar 0.9051)."""
    tgt, finals = mini_target(), {}
    for groups in (False, True):
        with S2D.Trainer(268, 213, 1024, deterministic=True) as t:
            t.set_target(tgt)
            t.init()
            if groups:
                g = R.GAIN_RATES
                t.set_optim(pos=g[0], scale=g[1], rot=g[2], color=g[3], opacity=g[4])
            mse = t.step(300)
            assert np.isfinite(mse).all()
            finals[groups] = mse[-1]
    ratio = finals[True] / finals[False]
    print("plain %.4f  group rates %.4f  ratio %.4f  (oracle %.4f / %.4f = %.4f, bar %.4f)" %
          (finals[False], finals[True], ratio, ORACLE_GROUPS, ORACLE_PLAIN, ORACLE_GROUPS / ORACLE_PLAIN, GAIN_BAR))
    assert ratio <= GAIN_BAR, (ratio, GAIN_BAR)


# ---------------------------------------------------------------------------------------------------------------------
# 9: refusals, the host tool
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_on_a_live_context():
    def refused(call, *a, **kw):
        with pytest.raises(S2D.S2DError) as e:
            call(*a, **kw)
        assert e.value.code == S2D_E_INVALID, (a, kw)

    with T.rig(W0, H0, 40, bind=False) as r:
        t = r.t
        for bad in (0.0, -0.05, float("inf"), float("nan")):
            for group in S2D.OPTIM_GROUPS:
                refused(t.set_optim, **{group: bad})
        for bad in (-0.5, float("inf"), float("nan")):
            for g in range(5):
                ratios = [0.5] * 5
                ratios[g] = bad
                refused(t.set_optim, pos=0.5, final_ratio=ratios, decay_iterations=10)
                refused(t.set_optim, pos=0.5, final_ratio=ratios)                  # (T = 0: the ratios are still validated)
        refused(t.set_optim, pos=0.5, decay_iterations=-1)
        refused(t.rates_at, -1)
        import ctypes as C
        cfg = S2D._OptimConfig()
        cfg.struct_size = C.sizeof(S2D._OptimConfig) - 4
        for g in range(5):
            cfg.rate[g] = 0.05
        assert t.L.s2d_set_optim(t._h, C.byref(cfg)) == S2D_E_INVALID
        assert t.rates_at(0).tobytes() == np.full(5, 0.05, dtype=F).tobytes()      # nothing of the refused ones stuck
        # a held set: all four calls, and slab ownership refuses a context under the controls
        masks = r.dev(np.full(40, 2, dtype=np.int32))
        t.halo_commit(masks.data_ptr(), 1)
        refused(t.set_optim, pos=0.5)
        refused(t.set_optim, None)
        refused(t.rates_at, 0)
        refused(t.set_frozen, np.zeros(40, dtype=bool))
        refused(t.set_frozen, None)
        refused(t.set_frozen_device, masks.data_ptr())
        t.halo_commit(0, 1)
        t.set_optim(pos=0.5)
        refused(t.halo_commit, masks.data_ptr(), 1)
        t.set_optim(None)
        t.set_frozen(np.zeros(40, dtype=bool))
        refused(t.halo_commit, masks.data_ptr(), 1)
        t.set_frozen(None)
        t.halo_commit(masks.data_ptr(), 1)
    with S2D.Trainer(64, 64, 10, row_begin=16, row_end=48) as slab:                # a slab context
        refused(slab.set_optim, pos=0.5)
        refused(slab.rates_at, 0)
        refused(slab.set_frozen, np.zeros(10, dtype=bool))
        refused(slab.set_frozen_device, 0)


def test_host_tool_group_rates_and_freeze_unmoved(tmp_path):
    exe = S2D._build.TRAIN_BIN
    base = [exe, "--image", MINI, "--splats", "1024", "--deterministic"]

    def run(extra):
        r = subprocess.run(base + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
        assert r.returncode == 0, r.stderr
        return r.stdout, r.stderr

    def final(out):
        return float(re.findall(r"^\d+ itr, mse ([0-9.]+)$", out, flags=re.M)[-1])

    plain, _ = run(["--iters", "120"])
    same, _ = run(["--iters", "120", "--lr-groups", "0.05,0.05,0.05,0.05,0.05"])
    assert same == plain and plain.count("\n") == 120                              # line for line
    groups, _ = run(["--iters", "120", "--lr-groups", "0.5,0.2,0.1,0.05,0.05", "--rebin-margin", "4.7"])
    assert final(groups) < final(plain)
    decayed, _ = run(["--iters", "120", "--lr-groups", "0.5,0.2,0.1,0.05,0.05", "--lr-final-ratio", "0.1,0.5,1,1,1", "--lr-decay-iters", "100"])
    assert decayed.splitlines()[:2] == groups.splitlines()[:2] and decayed != groups and np.isfinite(final(decayed))

    # --freeze-unmoved: the state in front of the reseeding at iteration 20, and ten iterations behind it
    def ckpt(iters, extra):
        path = str(tmp_path / ("ck%d%s" % (iters, "f" if extra else "")))
        _, err = run(["--iters", str(iters), "--quiet", "--reseed-every", "20", "--reseed-window", "3", "--reseed-min-weight", "1e30",
                      "--save-checkpoint", path] + extra)
        raw = np.fromfile(path, dtype=np.uint8)[28:]                                # CkptHeader: 28 bytes
        return raw[:1024 * 36].reshape(1024, 36), raw[1024 * 36:].reshape(1024, 72), err

    sp20, ad20, _ = ckpt(20, [])
    sp30, ad30, err = ckpt(30, ["--freeze-unmoved"])
    assert re.findall(r"reseeded (\d+) splats before iteration (\d+)", err) == [("102", "20")]
    assert "froze 922 splats, 102 stay trained" in err
    kept = (sp20 == sp30).all(axis=1) & (ad20 == ad30).all(axis=1)
    assert kept.sum() == 922                                                        # the unwritten rows, byte for byte
    sp30u, _, _ = ckpt(30, [])
    assert (sp20 == sp30u).all(axis=1).sum() < kept.sum() // 2                      # without the flag the visible rows train on
