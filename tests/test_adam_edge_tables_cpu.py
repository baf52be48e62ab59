"""The premises of tests/test_gpu_adam_step.py, checked without a GPU.

The GPU file compares adam_kernel with the oracle's s2do_adam_step on the tables of tests/adam_cases.py and expects
identical bytes.  That is only worth something if
  * the oracle does on those tables what the GPU file assumes (status 0 and finite state on the finite table; status 1 /
    NaN stored where the reference aborts / carries on) -- asserted here;
  * the oracle itself is right on them: a numpy restatement of main.cpp:144-156 and the clamps (:741-749), written
    independently of the C, must give the oracle's bytes;
  * the arithmetic the kernels are built from (adam_optimize of csrc/s2d_math.h, compiled for the host by
    tests/hostcheck) gives the oracle's bytes on every (value, m, v, g, betas) of the tables, in both forms of the quotient.
"""
import numpy as np
import pytest

import adam_cases as A
import hostcheck_lib
import oracle_lib as O

F = np.float32
MODES = [False, True]  # fp32 quotient (S2D_CFG_ADAM_FP32) off / on


@pytest.fixture(scope="module")
def hc():
    return hostcheck_lib.load()


# ---------------------------------------------------------------------------------------------------------------------
# main.cpp:144-156 and :741-749 in numpy: every line one IEEE operation on float32 (float64 where the reference's
# expression is evaluated in double), elementwise over the (n, 9) arrays.
# ---------------------------------------------------------------------------------------------------------------------
def numpy_adam(value, m, v, g, lr, b1t, b2t, fp32):
    with np.errstate(all="ignore"):
        one, e = F(1.0), F(1.0e-15)
        m = F(0.9) * m + (one - F(0.9)) * g
        v = F(0.99) * v + (one - F(0.99)) * g * g
        m_hat = m / (one - b1t)
        v_hat = v / (one - b2t)
        sm = lr * m_hat
        if fp32:
            out = value - sm / (np.sqrt(v_hat) + e)
        else:
            out = (value.astype(np.float64) - sm.astype(np.float64) / (np.sqrt(v_hat.astype(np.float64)) + np.float64(e))).astype(F)
    return out, m, v


def numpy_clamp(x, lo, hi):
    t = np.where(x < lo, lo, x)       # glm::max(x, lo)
    return np.where(hi < t, hi, t)    # glm::min(t, hi): a NaN stays


def numpy_step(splats, adams, grads, W, H, b1t, b2t, optimize_opacity, fp32):
    """-> (splats, adams, beta1t, beta2t, status) after main.cpp:714-785."""
    b1t, b2t = F(b1t * A.BETA1), F(b2t * A.BETA2)
    out, m, v = numpy_adam(splats, adams[..., 0], adams[..., 1], grads, A.LR, b1t, b2t, fp32)
    new_adams = np.stack([m, v], axis=2)
    if not optimize_opacity:
        out[:, 8] = splats[:, 8]
        new_adams[:, 8] = adams[:, 8]
    for k, b in enumerate(A.clamp_bounds(W, H)):
        if b is not None:
            out[:, k] = numpy_clamp(out[:, k], b[0], b[1])
    status = 0 if np.isfinite(out[:, list(A.GUARDED)]).all() else 1
    return out.astype(F), new_adams.astype(F), b1t, b2t, status


def hc_step(hc, splats, adams, grads, W, H, b1t, b2t, optimize_opacity, fp32):
    """The same step through adam_optimize of csrc/s2d_math.h (host build), scalar by scalar; clamps as above."""
    b1t, b2t = F(b1t * A.BETA1), F(b2t * A.BETA2)
    out, mv = np.array(splats, dtype=F), np.array(adams, dtype=F)
    hc.hc_adam_n(O._p(out), O._p(mv), O._p(np.ascontiguousarray(grads, dtype=F)), out.size, float(A.LR), float(b1t), float(b2t), int(fp32))
    if not optimize_opacity:
        out[:, 8] = splats[:, 8]
        mv[:, 8] = adams[:, 8]
    for k, b in enumerate(A.clamp_bounds(W, H)):
        if b is not None:
            out[:, k] = numpy_clamp(out[:, k], b[0], b[1])
    return out, mv


def check_all_three(hc, o, grads, optimize_opacity, want_status=None, what=""):
    """One oracle step of `o` on `grads`; the numpy restatement and the shared header from the same state must give its bytes."""
    s0, a0, b1, b2 = o.splats.copy(), o.adams.copy(), o.beta1t[0], o.beta2t[0]
    st = o.step(grads, optimize_opacity)
    if want_status is not None:
        assert st == want_status, (what, st)
    ns, na, nb1, nb2, nst = numpy_step(s0, a0, grads, o.W, o.H, b1, b2, optimize_opacity, o.fp32)
    assert nst == st, what
    assert A.bits(nb1) == A.bits(o.beta1t[0]) and A.bits(nb2) == A.bits(o.beta2t[0]), what
    A.assert_same_bits(ns, o.splats, what + " numpy splats")
    A.assert_same_bits(na, o.adams, what + " numpy moments")
    hs, ha = hc_step(hc, s0, a0, grads, o.W, o.H, b1, b2, optimize_opacity, o.fp32)
    A.assert_same_bits(hs, o.splats, what + " s2d_math.h splats")
    A.assert_same_bits(ha, o.adams, what + " s2d_math.h moments")
    return st, s0, a0


@pytest.mark.parametrize("fp32", MODES)
def test_finite_table_stays_finite_and_three_restatements_agree(hc, fp32):
    """Every size and image of the premise, six steps with the opacity flag alternating: the oracle reports status 0, all
    parameters and moments stay finite, about four scalars in ten change per step and hundreds of moments are denormal
    (so the table does reach what it is for)."""
    for (W, H) in A.IMAGES:
        for n in A.SIZES:
            t = A.finite_table(n, W, H)
            o = A.OracleState(t.splats, t.adams, W, H, fp32=fp32)
            changed, denormal = [], 0
            for s in range(t.grads.shape[0]):
                what = "%dx%d n=%d step %d fp32=%s" % (W, H, n, s, fp32)
                _, s0, _ = check_all_three(hc, o, t.grads[s], s % 2 == 1, want_status=0, what=what)
                assert np.isfinite(o.splats).all() and np.isfinite(o.adams).all(), what
                changed.append(float((A.bits(o.splats) != A.bits(s0)).mean()))
                denormal += int(((o.adams != 0) & (np.abs(o.adams) < A.FLT_MIN)).sum())
            if n >= 255:
                assert 0.2 < np.mean(changed) < 0.6, (W, H, n, changed)
                assert denormal >= 100, (W, H, n, denormal)
            # the zero-gradient share of the table
            zero_rows = (t.grads == 0).all(axis=2).mean()
            if n >= 255:
                assert 0.3 < zero_rows < 0.5, zero_rows


def test_beta_power_constants():
    """BETA_1200 is what 1200 multiplications leave: four denormal units (a fixed point of x * 0.9 under rounding), 5.78e-6."""
    b1, b2 = A.beta_powers(1200)
    assert A.bits(b1) == A.bits(A.BETA_1200[0]) == 4
    assert A.bits(b2) == A.bits(A.BETA_1200[1]) and abs(float(b2) - 5.78e-6) < 1e-8


@pytest.mark.parametrize("fp32", MODES)
def test_beta_powers_stay_finite(hc, fp32):
    for (b1, b2, it) in A.BETAS:
        t = A.finite_table(257, 37, 21, steps=2)
        o = A.OracleState(t.splats, t.adams, 37, 21, b1, b2, it, fp32=fp32)
        for s in range(2):
            check_all_three(hc, o, t.grads[s], s % 2 == 1, want_status=0, what="betas %r step %d" % ((b1, b2, it), s))
            assert np.isfinite(o.splats).all() and np.isfinite(o.adams).all()


@pytest.mark.parametrize("fp32", MODES)
@pytest.mark.parametrize("layout", A.DORMANT_LAYOUTS)
def test_dormant_layouts(hc, fp32, layout):
    """Layout 1: the reference does not leave the zero block as it is (a -0.0 first moment meets a +0 gradient and becomes
    +0, a -0.0 parameter loses its sign with it), and -0.0 moments and gradients are there before every step.  Layout 3:
    moments and gradients of the block are +0 bit for bit before both wake-up steps, so a kernel that skips blocks of +0
    moments under +0 gradients has skipped this one, and each wake-up is the only gradient the block receives."""
    t = A.dormant_table(layout)
    o = A.OracleState(t.splats, t.adams, t.W, t.H, fp32=fp32)
    rows, wakes = A.DORMANT_ROWS, (A.DORMANT_WAKE, A.DORMANT_WAKE_NEGATIVE)
    moved = 0
    for s in range(t.grads.shape[0]):
        before = o.adams[rows].copy()
        if layout == 3:
            assert not A.bits(before).any(), s
            g = t.grads[s, rows].copy()
            for ws, row, k, val in wakes:
                if ws == s:
                    assert A.bits(g[row - rows.start, k]) == A.bits(val) != 0
                    g[row - rows.start, k] = 0.0
            assert not A.bits(g).any(), s
        if layout == 1:
            assert (A.bits(before) != 0).any() and (A.bits(t.grads[s, rows]) != 0).any(), s
        p0 = o.splats[rows].copy()
        check_all_three(hc, o, t.grads[s], s % 2 == 1, want_status=0, what="layout %d step %d" % (layout, s))
        assert (o.adams[rows] == 0).all() or s >= A.DORMANT_WAKE[0]
        moved += int((A.bits(o.adams[rows]) != A.bits(before)).sum())
        if layout == 3 and s == A.DORMANT_WAKE_NEGATIVE[0]:
            row = A.DORMANT_WAKE_NEGATIVE[1] - rows.start   # the negative wake-up changes the row's state: a skip shows
            assert (A.bits(o.adams[rows][row]) != 0).any() and (A.bits(o.splats[rows][row]) != A.bits(p0[row])).any()
    assert (moved > 0) == (layout != 2)


@pytest.mark.parametrize("fp32", MODES)
def test_nonfinite_gradients_status_per_field(hc, fp32):
    """Nine fields x (+inf, -inf, NaN): the reference aborts for seven fields; for pos.y and opacity it stores a NaN and
    carries on, and with the opacity flag off the opacity is untouched."""
    for field, name in A.NONFINITE_CASES:
        t = A.nonfinite_table(field, name)
        for flag in (True, False):
            o = A.OracleState(t.splats, t.adams, t.W, t.H, fp32=fp32)
            what = "%s %s flag=%s" % (A.FIELDS[field], name, flag)
            check_all_three(hc, o, t.grads[0], flag, want_status=A.nonfinite_status(field), what=what)
            row = o.splats[A.NONFINITE_ROW]
            if field == 8 and not flag:
                assert A.bits(row[8]) == A.bits(numpy_clamp(t.splats[A.NONFINITE_ROW, 8], F(0.1), F(1.0))), what
                assert np.isfinite(o.splats).all(), what
            else:
                assert np.isnan(row[field]), what
                assert np.isnan(o.splats).sum() == 1, what


@pytest.mark.parametrize("fp32", MODES)
def test_overflow_table_status(hc, fp32):
    for name, fields, status in A.OVERFLOW_CASES:
        t = A.overflow_table(fields)
        assert np.isfinite(t.splats).all() and np.isfinite(t.adams).all() and np.isfinite(t.grads).all()
        o = A.OracleState(t.splats, t.adams, t.W, t.H, fp32=fp32)
        check_all_three(hc, o, t.grads[0], True, want_status=status, what="overflow, " + name)
        assert np.isnan(o.splats[list(A.OVERFLOW_ROWS)][:, list(fields)]).all(), name
