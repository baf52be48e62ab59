"""adam_kernel (csrc/s2d_optim.hip) against the oracle's s2do_adam_step on injected gradients: identical bytes.

No raster pass is involved: s2d_adam_step runs on whatever the gradient buffer holds, and the buffer is a torch tensor
bound with s2d_bind_grads_device (or written with s2d_rows_scatter(S2D_ROWS_GRADS)), so the gradients are the tables of
tests/adam_cases.py -- signed zeros, denormals, the float extremes, infinities, NaN -- which no backward pass produces.
tests/test_adam_edge_tables_cpu.py asserts what these tests assume about the oracle on the same tables.

Every comparison goes through `same_state`: parameters (n x 9), moments (n x 18), beta1t, beta2t and the iteration count
from s2d_get_splats / s2d_get_adam against the oracle's; NaN in the same places, every other scalar with the same bits
(-0 is not +0); and after a step of a whole context the gradient buffer is all zero bits (main.cpp:550 value-initialises
dSplats every iteration).

The contexts work on torch's current stream, so torch's copies into the gradient buffer and the library's launches are
ordered without host synchronisation (needed where several steps are queued behind one another).
"""
import contextlib
import importlib

import numpy as np
import pytest

import adam_cases as A
import oracle_lib as O

pytestmark = pytest.mark.gpu

S2D = importlib.import_module("2dgaussiansplatting_amd")
F = np.float32
W0, H0 = 37, 21
S2D_E_NONFINITE = 3


class Rig:
    """A context on torch's current stream and the gradient tensor bound to it."""

    def __init__(self, t, torch, bind):
        self.t, self.torch, self.n = t, torch, t.n
        self.g = None
        if bind:
            self.g = torch.zeros((t.n, 9), dtype=torch.float32, device="cuda")
            t.bind_grads(self.g.data_ptr())

    def dev(self, a, dtype=None):
        x = self.torch.from_numpy(np.ascontiguousarray(a))
        return (x if dtype is None else x.to(dtype)).cuda()

    def load(self, o):
        """The oracle's state into the context (also clears a non-finite condition, include/splat2d.h)."""
        self.t.set_splats(o.splats.view(S2D.SPLAT_DTYPE).reshape(-1))
        self.t.set_adam(o.adams.reshape(-1, 18).view(S2D.ADAM_DTYPE).reshape(-1), o.beta1t[0], o.beta2t[0], o.iterations)

    def inject(self, grads):
        self.g.copy_(self.torch.from_numpy(np.ascontiguousarray(grads, dtype=F)))

    def step(self, grads, optimize_opacity):
        self.inject(grads)
        self.t.optimize_opacity = bool(optimize_opacity)
        self.t.adam_step()

    def grads(self):
        return self.g.cpu().numpy()

    def state(self):
        sp = self.t.get_splats().view(F).reshape(self.n, 9)
        ad, b1, b2, it = self.t.get_adam()
        return sp, ad.view(F).reshape(self.n, 9, 2), b1, b2, it


@contextlib.contextmanager
def rig(W, H, n, bind=True, **kw):
    import torch
    with torch.cuda.stream(torch.cuda.Stream()):
        with S2D.Trainer(W, H, n, stream=torch.cuda.current_stream().cuda_stream, **kw) as t:
            yield Rig(t, torch, bind)
            torch.cuda.current_stream().synchronize()


def same_state(r, o, what, grads_zero=True):
    """THE comparison: everything s2d_get_splats / s2d_get_adam return against the oracle's, bit for bit."""
    sp, ad, b1, b2, it = r.state()
    A.assert_same_bits(sp, o.splats, what + ": parameters")
    A.assert_same_bits(ad, o.adams, what + ": moments")
    assert A.bits(b1) == A.bits(o.beta1t[0]) and A.bits(b2) == A.bits(o.beta2t[0]), (what, b1, b2, o.beta1t, o.beta2t)
    assert it == o.iterations, (what, it, o.iterations)
    if grads_zero:
        left = A.bits(r.grads() if r.g is not None else r.t.get_grads().view(F))
        assert not left.any(), "%s: %d gradient scalars are not +0 after the step" % (what, int((left != 0).sum()))


def run_table(r, t, o, what, flags=None):
    """Step context and oracle through the table's gradients, comparing after every step; the oracle stays at status 0."""
    for s in range(t.grads.shape[0]):
        flag = (s % 2 == 1) if flags is None else flags[s]
        assert o.step(t.grads[s], flag) == 0
        r.step(t.grads[s], flag)
        r.t.synchronize()
        same_state(r, o, "%s, step %d" % (what, s))


# ---------------------------------------------------------------------------------------------------------------------
# sizes and tails
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp32", [False, True])
@pytest.mark.parametrize("n", [1, 3, 255, 256, 257, 777])
def test_finite_table_sizes_and_tails(n, fp32):
    """9 n and 18 n are multiples of four only for some of these n (the float4 body and the dword tail of lds_fill /
    lds_drain), 255 / 256 / 257 sit around the block size, 777 leaves a partial fourth block."""
    t = A.finite_table(n, W0, H0)
    o = A.OracleState(t.splats, t.adams, W0, H0, fp32=fp32)
    with rig(W0, H0, n, adam_fp32=fp32) as r:
        r.load(o)
        run_table(r, t, o, "n=%d fp32=%s" % (n, fp32))


def test_finite_table_wide_image():
    """W = 4096: the pos.x clamp at 4095, its neighbour below, and 4105 outside."""
    W, H, n = 4096, 64, 257
    t = A.finite_table(n, W, H)
    assert (t.splats[:, 0] == F(4095)).any() and (t.splats[:, 0] == F(4105)).any()
    o = A.OracleState(t.splats, t.adams, W, H)
    with rig(W, H, n) as r:
        r.load(o)
        run_table(r, t, o, "4096x64")


@pytest.mark.parametrize("case", range(len(A.BETAS)))
def test_beta_powers(case):
    """beta1t = beta2t = 1 (the first step), a denormal beta1t, zero, and one step in: 1 - beta?t as the divisor."""
    b1, b2, it = A.BETAS[case]
    n = 257
    t = A.finite_table(n, W0, H0, steps=2)
    o = A.OracleState(t.splats, t.adams, W0, H0, b1, b2, it)
    with rig(W0, H0, n) as r:
        r.load(o)
        run_table(r, t, o, "betas %r" % ((b1, b2, it),))


# ---------------------------------------------------------------------------------------------------------------------
# dormant blocks
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", A.DORMANT_LAYOUTS)
def test_dormant_block_is_skipped_only_where_the_reference_changes_nothing(layout):
    """One whole block of zero gradients over zero moments.  The oracle skips nothing, so a block the kernel must not skip
    shows as a byte: with signed zeros mixed (layouts 1 and 2) a -0.0 moment that the reference turns into +0, a -0.0
    gradient left in the buffer; with +0 only (layout 3) the block sleeps for three steps and is then woken by one
    denormal gradient -- left in the buffer if the block is skipped again -- and a step later by one negative gradient."""
    t = A.dormant_table(layout)
    o = A.OracleState(t.splats, t.adams, t.W, t.H)
    with rig(t.W, t.H, t.n) as r:
        r.load(o)
        run_table(r, t, o, "dormant layout %d" % layout)


def test_init_then_step_with_zero_gradients():
    W, H, n = 268, 213, 777
    ot = O.OracleTrainer(np.zeros((H, W, 4), dtype=F), n)
    o = A.OracleState(ot.splats.view(F).reshape(n, 9), ot.adams.view(F).reshape(n, 9, 2), W, H)
    zero = np.zeros((n, 9), dtype=F)
    with rig(W, H, n) as r:
        r.t.init()
        same_state(r, o, "init")
        for s in range(2):
            assert o.step(zero, s == 1) == 0
            r.t.optimize_opacity = s == 1
            r.t.adam_step()
            r.t.synchronize()
            same_state(r, o, "init, step %d" % s)


# ---------------------------------------------------------------------------------------------------------------------
# finite guard
# ---------------------------------------------------------------------------------------------------------------------
def guard_case(r, t, flag, want_status, what, start=5):
    """One step from iteration `start`: S2D_E_NONFINITE exactly where the oracle returns 1, with the iteration the step ran
    as in the statistics; the state is the oracle's either way."""
    o = A.OracleState(t.splats, t.adams, t.W, t.H, *A.beta_powers(start), start)
    r.load(o)
    assert o.step(t.grads[0], flag) == want_status, what
    r.step(t.grads[0], flag)
    if want_status:
        with pytest.raises(S2D.S2DError) as e:
            r.t.synchronize()
        assert e.value.code == S2D_E_NONFINITE, what
        assert r.t.stats()["first_nonfinite_iteration"] == start, what
    else:
        r.t.synchronize()
        assert r.t.stats()["first_nonfinite_iteration"] == -1, what
    same_state(r, o, what)
    return o


def test_finite_guard_nonfinite_gradients():
    """Nine fields x (+inf, -inf, NaN) in a row of the second block.  Seven fields abort; pos.y and opacity store the NaN
    and carry on (main.cpp:752-785 does not look at them); with the opacity flag off the opacity is not touched at all."""
    with rig(W0, H0, 300) as r:
        for field, name in A.NONFINITE_CASES:
            t = A.nonfinite_table(field, name)
            what = "%s gradient %s" % (A.FIELDS[field], name)
            o = guard_case(r, t, True, A.nonfinite_status(field), what)
            assert np.isnan(o.splats[A.NONFINITE_ROW, field])
            if field == 8:
                o = guard_case(r, t, False, 0, what + ", flag off")
                assert np.isfinite(o.splats).all() and A.bits(o.adams[:, 8]).tolist() == A.bits(t.adams[:, 8]).tolist()


def test_finite_guard_overflow_table():
    """Finite inputs at +-FLT_MAX: g * g and m / (1 - beta1t) overflow, the quotient is inf / inf."""
    with rig(W0, H0, 300) as r:
        for name, fields, status in A.OVERFLOW_CASES:
            guard_case(r, A.overflow_table(fields), True, status, "overflow, " + name)


def test_steps_queued_behind_a_nonfinite_one_do_nothing():
    """Three steps queued, the first one non-finite: the state is the oracle's after ONE step, the counters are wound back
    to it (judge_status), and the gradients handed to steps two and three are still in the buffer."""
    start, n = 5, 300
    t = A.nonfinite_table(2, "+inf")
    later = A.finite_table(n, W0, H0, steps=2, seed=31).grads
    assert A.bits(later).any(axis=1).all()  # (every row distinguishable from a consumed, zeroed one)
    o = A.OracleState(t.splats, t.adams, W0, H0, *A.beta_powers(start), start)
    with rig(W0, H0, n) as r:
        r.load(o)
        assert o.step(t.grads[0], True) == 1
        r.step(t.grads[0], True)
        r.step(later[0], True)
        after_two = r.g.clone()
        r.step(later[1], True)
        with pytest.raises(S2D.S2DError) as e:
            r.t.synchronize()
        assert e.value.code == S2D_E_NONFINITE
        assert r.t.stats()["first_nonfinite_iteration"] == start
        assert o.iterations == start + 1
        same_state(r, o, "queued behind a non-finite step", grads_zero=False)
        assert A.bits(after_two.cpu().numpy()).tolist() == A.bits(later[0]).tolist()
        assert A.bits(r.grads()).tolist() == A.bits(later[1]).tolist()


# ---------------------------------------------------------------------------------------------------------------------
# held sets (s2d_halo_commit): the ids-indexed path and the compact copy
# ---------------------------------------------------------------------------------------------------------------------
HELD_N = 1000


def held_mask(name):
    m = np.zeros(HELD_N, dtype=bool)
    if name == "every other":
        m[0::2] = True
    elif name == "one":
        m[999] = True
    elif name == "257 random":
        m[np.random.default_rng(257).permutation(HELD_N)[:257]] = True
    elif name == "all":
        m[:] = True
    return m  # "none": nothing held


SCATTERED = np.array([[3.0, 4.0, 2.0, 7.0, 0.5, 0.2, 0.4, 0.6, 0.8],
                      [46.0, -5.0, 0.25, 5000.0, -0.0, -1.0, 2.0, 0.5, 7.0]], dtype=F)  # second row: outside the clamps


@pytest.mark.parametrize("compact", ["default", "0"])
@pytest.mark.parametrize("mask_name", ["every other", "one", "257 random", "all", "none"])
def test_held_set_updates_exactly_the_held_records(monkeypatch, mask_name, compact):
    """Expected: the oracle's step on the held rows gathered, scattered back; every other parameter, moment and gradient
    row byte-identical to before.  Between steps two and three one held and one non-held row are rewritten through
    s2d_rows_scatter (which reloads the compact copy); s2d_get_splats / s2d_get_adam flush it."""
    if compact == "default":
        monkeypatch.delenv("S2D_COMPACT_HELD", raising=False)
    else:
        monkeypatch.setenv("S2D_COMPACT_HELD", compact)
    n, rank = HELD_N, 1
    mask = held_mask(mask_name)
    idx = np.nonzero(mask)[0]
    t = A.finite_table(n, W0, H0, steps=4)
    exp_s, exp_a = t.splats.copy(), t.adams.copy()
    b1, b2, it = F(1.0), F(1.0), 0
    with rig(W0, H0, n) as r:
        r.load(A.OracleState(exp_s, exp_a, W0, H0))
        masks = r.dev(mask.astype(np.int32) << rank)
        r.t.halo_commit(masks.data_ptr(), rank)
        for s in range(4):
            if s == 2:
                rows = [int(i[len(i) // 2]) for i in (idx, np.nonzero(~mask)[0]) if len(i)]
                vals = SCATTERED[:len(rows)] if len(idx) else SCATTERED[1:]
                ids, new = r.dev(np.array(rows, dtype=np.int32)), r.dev(vals)
                r.t.rows_scatter(S2D.ROWS_SPLATS, ids.data_ptr(), len(rows), new.data_ptr())
                exp_s[rows] = vals
            flag = s % 2 == 1
            sub = A.OracleState(exp_s[idx], exp_a[idx], W0, H0, b1, b2, it)
            assert sub.step(t.grads[s][idx], flag) == 0
            exp_s[idx], exp_a[idx] = sub.splats, sub.adams
            b1, b2, it = sub.beta1t[0], sub.beta2t[0], sub.iterations
            exp_g = t.grads[s].copy()
            exp_g[idx] = 0.0
            r.step(t.grads[s], flag)
            r.t.synchronize()
            what = "held %s, compact %s, step %d" % (mask_name, compact, s)
            same_state(r, A.OracleState(exp_s, exp_a, W0, H0, b1, b2, it), what, grads_zero=False)
            assert A.bits(r.grads()).tolist() == A.bits(exp_g).tolist(), what


# ---------------------------------------------------------------------------------------------------------------------
# gradients written with s2d_rows_scatter(S2D_ROWS_GRADS) into the context's own buffer
# ---------------------------------------------------------------------------------------------------------------------
def test_gradients_through_rows_scatter():
    n = 257
    t = A.finite_table(n, W0, H0, steps=4)
    o = A.OracleState(t.splats, t.adams, W0, H0)
    with rig(W0, H0, n, bind=False) as r, rig(W0, H0, n) as bound:
        r.load(o)
        bound.load(o)
        ids = r.dev(np.arange(n, dtype=np.int32))
        for s in range(4):
            flag = s % 2 == 1
            assert o.step(t.grads[s], flag) == 0
            vals = r.dev(t.grads[s])
            r.t.rows_scatter(S2D.ROWS_GRADS, ids.data_ptr(), n, vals.data_ptr())
            r.t.optimize_opacity = flag
            r.t.adam_step()
            r.t.synchronize()
            same_state(r, o, "rows_scatter gradients, step %d" % s)
            bound.step(t.grads[s], flag)
            bound.t.synchronize()
            got, want = r.state(), bound.state()
            A.assert_same_bits(got[0], want[0], "scattered against bound: parameters")
            A.assert_same_bits(got[1], want[1], "scattered against bound: moments")


# ---------------------------------------------------------------------------------------------------------------------
# the projection fused into the step
# ---------------------------------------------------------------------------------------------------------------------
def test_fused_projection_after_a_wild_update():
    """With re-usable lists the step also projects what it wrote and checks it against the binned rectangles.  Starting
    from init() (parameters a forward pass can render), the finite table's moments and gradients throw positions and sizes
    across the image in one step; the next forward() must be the oracle's forward of the oracle's post-step parameters,
    bit for bit.  On a context that owns the whole image such an update trips the containment check and the lists are
    rebuilt: that is what is tested; the empty record for a splat that left a row slab is not reached here.  rot, which
    is not clamped, gets moments and gradients of ordinary size and is asserted to stay within |rot| < 120, the range in
    which sin / cos -- and so the forward pass -- are bitwise by construction (csrc/s2d_math.h, sincos_f32)."""
    W, H, n = 96, 80, 300
    tgt = O.synthetic_target(W, H)
    ot = O.OracleTrainer(tgt, n)
    t = A.finite_table(n, W, H, steps=2, seed=5)
    rng = np.random.default_rng(5)
    t.adams[:, 4, 0] = np.array([0.0, -0.0, 0.3, -2.0], dtype=F)[rng.integers(0, 4, n)]
    t.adams[:, 4, 1] = np.array([0.3, 4.0], dtype=F)[rng.integers(0, 2, n)]
    t.grads[:, :, 4] = np.array([0.0, -0.0, 1e-8, -3e-4, 1.0, -7.5], dtype=F)[rng.integers(0, 6, (2, n))]
    start = ot.splats.view(F).reshape(n, 9).copy()
    o = A.OracleState(start, t.adams, W, H)
    with rig(W, H, n, rebin_interval=8) as r:
        r.t.set_target_synthetic()
        r.load(o)
        r.t.forward()
        assert r.t.get_image().tobytes() == ot.forward().tobytes()
        for s in range(2):
            assert o.step(t.grads[s], s == 1) == 0
            r.step(t.grads[s], s == 1)
            r.t.forward()
            r.t.synchronize()
            assert (np.abs(o.splats[:, 4]) < 120).all()
            ot.splats[:] = o.splats.view(O.SPLAT_DTYPE).reshape(-1)
            assert r.t.get_image().tobytes() == ot.forward().tobytes(), "round %d" % s
            same_state(r, o, "fused projection, round %d" % s)
        assert (np.abs(o.splats[:, 0] - start[:, 0]) > 20).any()  # (wild: across a quarter of the image in two steps)
