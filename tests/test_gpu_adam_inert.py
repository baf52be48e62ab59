"""adam_kernel (csrc/s2d_optim.hip) skips INERT splats one by one: a splat whose nine gradient words and eighteen moments are
all +0 is neither loaded nor stored, a 16-byte line of the block's arrays moves only when a live record has words on it,
and a skipped splat keeps its projection record -- which is only right while that record was made from its parameters.

Everything is compared the way tests/test_gpu_adam_step.py compares (its `rig` and `same_state`): parameters, moments,
beta powers and the iteration count bytes-equal to the oracle's s2do_adam_step, which skips nothing; the gradient buffer
all +0 afterwards.  The first step after a state is loaded runs every splat (loading clears what the kernel knows about
the moments), so the skip is at work from the second step of a table on: four steps each.

Inert and live records are mixed in patterns that put them on shared lines in every phase (36- and 72-byte records
against 16-byte lines: the phase repeats every four records), at sizes around one and two blocks of 256.  A record that
wrongly sleeps shows as a live row that did not move or a gradient left in the buffer; a line moved with stale or foreign
words shows in the inert neighbour's bytes.
"""
import numpy as np
import pytest

import adam_cases as A
import oracle_lib as O
import test_gpu_adam_step as T

pytestmark = pytest.mark.gpu

S2D = T.S2D
F = np.float32
W1, H1 = 268, 213
STEPS = 4
SIZES = (255, 256, 257, 513, 1000)
PATTERNS = ("alternating", "runs of 1-7", "one live per block", "one inert per block", "all inert", "all live")
SIX_DENORMAL_UNITS = np.array([6], dtype=np.uint32).view(F)[0]  # 0.9 * 6 units rounds to 5: a moment that still moves


def live_mask(pattern, n):
    m = np.zeros(n, dtype=bool)
    if pattern == "alternating":
        m[0::2] = True
    elif pattern == "runs of 1-7":  # live and inert runs of 1, 2, ... 7, 1, ... records, taking turns
        at, run, live = 0, 1, True
        while at < n:
            m[at:at + run] = live
            at, run, live = at + run, run % 7 + 1, not live
    elif pattern in ("one live per block", "one inert per block"):
        m[:] = pattern == "one inert per block"
        for b in range((n + 255) // 256):  # first record of block 0, last of block 1, then wandering
            r = min(b * 256 + (0, 255, 130, 77)[b % 4], n - 1)
            m[r] = not m[r]
    elif pattern == "all live":
        m[:] = True
    return m


def inert_table(n, live, W=W1, H=H1, steps=STEPS, seed=40):
    """The finite table with the rows of ~live made inert (+0 moments, +0 gradients in every step) and every live row given a
    gradient in every step, so that a live row that was skipped cannot pass for one that had nothing to do."""
    t = A.finite_table(n, W, H, steps=steps, seed=seed)
    t.adams[~live] = 0.0
    t.grads[:, ~live] = 0.0
    for s in range(steps):
        idle = live & ~A.bits(t.grads[s]).any(axis=1)
        t.grads[s, idle, (s * 2) % 9] = (F(1e-8), F(-3e-4), F(1.0), F(-7.5))[s % 4]
    assert not A.bits(t.adams[~live]).any() and not A.bits(t.grads[:, ~live]).any()
    assert A.bits(t.grads[:, live]).any(axis=2).all()
    return t


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", SIZES)
def test_inert_and_live_records_mixed(n, pattern):
    t = inert_table(n, live_mask(pattern, n))
    o = A.OracleState(t.splats, t.adams, W1, H1)
    with T.rig(W1, H1, n) as r:
        r.load(o)
        T.run_table(r, t, o, "n=%d %s" % (n, pattern))


@pytest.mark.parametrize("pattern", ["all inert", "alternating"])
def test_almost_inert_records_run(pattern):
    """Asleep after the first step, then: row 100 gets one -0.0 gradient (the reference's sums start from +0: it must be
    replaced); row 301 carries one denormal first moment from the start (6 units -> 5 -> 4 -> 4: never dormant, and it
    moves); row 470 sleeps two steps and is then handed one denormal gradient, row 471 an ordinary one."""
    n = 513
    live = live_mask(pattern, n)
    rows = (100, 301, 470, 471)
    live[list(rows)] = False
    t = inert_table(n, live)
    t.grads[2, 100, 3] = F(-0.0)
    t.adams[301, 4, 0] = SIX_DENORMAL_UNITS
    t.grads[2, 470, 7] = A.DENORM_1
    t.grads[2, 471, 0] = F(-3e-4)
    o = A.OracleState(t.splats, t.adams, W1, H1)
    with T.rig(W1, H1, n) as r:
        r.load(o)
        before = o.adams[301, 4, 0]
        T.run_table(r, t, o, "almost inert, " + pattern)
        assert A.bits(o.adams[301, 4, 0]) != A.bits(before) and A.bits(o.adams[301, 4, 0]) != 0  # (it did move, and is not 0)
        assert A.bits(o.adams[471]).any()


# ---------------------------------------------------------------------------------------------------------------------
# held sets: the ids-indexed path and the compact copy
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compact", ["default", "0"])
def test_inert_records_in_a_held_set(monkeypatch, compact):
    """Every other splat held (500 of 1000: two blocks of the launch), live and inert in runs of 1-7 over the splat ids."""
    if compact == "default":
        monkeypatch.delenv("S2D_COMPACT_HELD", raising=False)
    else:
        monkeypatch.setenv("S2D_COMPACT_HELD", compact)
    n, rank = 1000, 1
    held = np.zeros(n, dtype=bool)
    held[0::2] = True
    idx = np.nonzero(held)[0]
    t = inert_table(n, live_mask("runs of 1-7", n), W=T.W0, H=T.H0)
    exp_s, exp_a = t.splats.copy(), t.adams.copy()
    b1, b2, it = F(1.0), F(1.0), 0
    with T.rig(T.W0, T.H0, n) as r:
        r.load(A.OracleState(exp_s, exp_a, T.W0, T.H0))
        masks = r.dev(held.astype(np.int32) << rank)
        r.t.halo_commit(masks.data_ptr(), rank)
        for s in range(STEPS):
            sub = A.OracleState(exp_s[idx], exp_a[idx], T.W0, T.H0, b1, b2, it)
            assert sub.step(t.grads[s][idx], s % 2 == 1) == 0
            exp_s[idx], exp_a[idx] = sub.splats, sub.adams
            b1, b2, it = sub.beta1t[0], sub.beta2t[0], sub.iterations
            exp_g = t.grads[s].copy()
            exp_g[idx] = 0.0
            r.step(t.grads[s], s % 2 == 1)
            r.t.synchronize()
            what = "held, compact %s, step %d" % (compact, s)
            T.same_state(r, A.OracleState(exp_s, exp_a, T.W0, T.H0, b1, b2, it), what, grads_zero=False)
            assert A.bits(r.grads()).tolist() == A.bits(exp_g).tolist(), what


# ---------------------------------------------------------------------------------------------------------------------
# the projection record of a skipped splat
# ---------------------------------------------------------------------------------------------------------------------
PW, PH, PN = 96, 80, 300
QUIET = np.arange(0, PN, 3)  # every third splat, the first of the blend order among them: zero gradients throughout


def proj_grads(steps, seed=9):
    """Ordinary gradients for everyone but QUIET."""
    rng = np.random.default_rng(seed)
    g = (rng.standard_normal((steps, PN, 9)) * 1e-3).astype(F)
    g[:, QUIET] = 0.0
    return g


def moved(splats):
    """Other parameters for QUIET: a few pixels aside, another colour."""
    s = splats.copy()
    s[QUIET, 0] = np.clip(s[QUIET, 0] + F(5.0), 0, PW - 1)
    s[QUIET, 1] = np.clip(s[QUIET, 1] - F(3.0), 0, PH - 1)
    s[QUIET, 5:8] = F(1.0) - s[QUIET, 5:8]
    return np.ascontiguousarray(s, dtype=F)


class ProjScene:
    """A context with re-usable lists and the oracle beside it, both at init(): launch A has run, with a forward before it."""

    def __init__(self, r):
        self.r, self.g = r, proj_grads(4)
        self.ot = O.OracleTrainer(O.synthetic_target(PW, PH), PN)
        self.o = A.OracleState(self.ot.splats.view(F).reshape(PN, 9), self.ot.adams.view(F).reshape(PN, 9, 2), PW, PH)
        r.t.set_target_synthetic()
        r.t.init()
        self.same_frame("init")
        self.launch(0)

    def launch(self, s, forward=False):
        assert self.o.step(self.g[s], False) == 0
        self.r.step(self.g[s], False)
        if forward:
            self.same_frame("launch %d" % s)

    def same_frame(self, what):
        self.r.t.forward()
        self.r.t.synchronize()
        self.ot.splats[:] = self.o.splats.view(O.SPLAT_DTYPE).reshape(-1)
        assert self.r.t.get_image().tobytes() == self.ot.forward().tobytes(), what
        T.same_state(self.r, self.o, what)


def test_skipped_splats_keep_a_current_projection():
    """Lists in re-use, a forward pass between the launches: QUIET is skipped from launch B on and drawn from the records
    launch A left."""
    with T.rig(PW, PH, PN, rebin_interval=8) as r:
        sc = ProjScene(r)
        for s in (1, 2, 3):
            sc.launch(s, forward=True)


@pytest.mark.parametrize("how", ["set_splats", "rows_scatter", "set_splats_device", "init", "set_adam"])
def test_parameters_replaced_between_two_launches(how):
    """Launch A on fresh parameters; QUIET's parameters (or everybody's) replaced while its gradients and moments stay +0;
    launch B; the forward pass must be the oracle's on the new parameters.  set_splats and init ask for new lists,
    rows_scatter and set_splats_device leave them in re-use (launch B projects), set_adam replaces no parameter."""
    with T.rig(PW, PH, PN, rebin_interval=8) as r:
        sc = ProjScene(r)
        o = sc.o
        if how == "init":
            sc.ot.init()
            sc.o = o = A.OracleState(sc.ot.splats.view(F).reshape(PN, 9), sc.ot.adams.view(F).reshape(PN, 9, 2), PW, PH)
            r.t.init()
        elif how == "set_adam":
            o.adams[1::3] = 0.0
            r.t.set_adam(o.adams.reshape(-1, 18).view(S2D.ADAM_DTYPE).reshape(-1), o.beta1t[0], o.beta2t[0], o.iterations)
        else:
            o.splats[:] = moved(o.splats)
            if how == "set_splats":
                r.t.set_splats(o.splats.view(S2D.SPLAT_DTYPE).reshape(-1))
            elif how == "rows_scatter":
                ids, new = r.dev(QUIET.astype(np.int32)), r.dev(o.splats[QUIET])
                r.t.rows_scatter(S2D.ROWS_SPLATS, ids.data_ptr(), len(QUIET), new.data_ptr())
            else:
                new = r.dev(o.splats)
                r.t.set_splats_device(new.data_ptr())
        sc.launch(1, forward=True)
        sc.launch(2, forward=True)


def test_two_launches_without_a_forward_pass_after_a_failed_containment_check():
    """QUIET's rows are scattered far outside the image with the lists in re-use.  Launch B clamps them to the right edge,
    out of their binned rectangles, and goes to sleep over them; launch C follows at once, finds them inert -- and must
    still leave the request for new lists standing, or the forward pass draws them through lists that do not name them."""
    with T.rig(PW, PH, PN, rebin_interval=8) as r:
        sc = ProjScene(r)
        sc.o.splats[QUIET, 0] = F(PW + 50)
        ids, new = r.dev(QUIET.astype(np.int32)), r.dev(sc.o.splats[QUIET])
        r.t.rows_scatter(S2D.ROWS_SPLATS, ids.data_ptr(), len(QUIET), new.data_ptr())
        sc.launch(1)
        sc.launch(2, forward=True)
        assert (sc.o.splats[QUIET, 0] == F(PW - 1)).all()
        sc.launch(3, forward=True)
