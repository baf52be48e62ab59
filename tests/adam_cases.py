"""Input tables for the Adam launch (adam_kernel, csrc/s2d_optim.hip) and the oracle's side of every comparison.

Shared by tests/test_adam_edge_tables_cpu.py (the premises, on the CPU) and tests/test_gpu_adam_step.py (the kernel).
The values are the ones a real backward pass never produces: signed zeros, denormals, the float extremes, parameters on
and beyond the clamp bounds, infinities and NaN.  Every array is float32; the rows are put together from the constants
below by a seeded generator, so both sides of a comparison, and both test files, see the same bytes.

The expected agreement between the library and the oracle is bytes-equal (assert_same_bits): both evaluate main.cpp:144-156
operation by operation without FMA contraction, with correctly rounded fp32 divide / sqrt and the same double quotient.
"""
import numpy as np

import oracle_lib as O

F = np.float32
FLT_MIN = F(1.17549435e-38)   # smallest normal
FLT_MAX = F(3.4028235e38)
DENORM_1 = F(1e-45)           # one unit of the denormal range (1.4e-45)
LR = F(0.05)                  # main.cpp:715, what a context uses unless told otherwise
BETA1, BETA2 = F(0.9), F(0.99)
FIELDS = ("pos.x", "pos.y", "sx", "sy", "rot", "col.r", "col.g", "col.b", "opacity")
GUARDED = (0, 2, 3, 4, 5, 6, 7)   # the fields main.cpp:752-785 looks at: not pos.y (1), not opacity (8)

# ---- the finite table -------------------------------------------------------------------------------------------------
GRADS = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, 1.17549435e-38, 1e-23, -1e-23, 1e-19, 1e-8, -3e-4, 1.0, -7.5, 1e15, -1e15],
                 dtype=F)
FIRST_MOMENTS = np.array([0.0, -0.0, 1e-45, -1e-40, 1e-30, 0.3, -2.0, 1e15], dtype=F)
SECOND_MOMENTS = np.array([0.0, 1e-45, 1e-40, 1e-30, 0.3, 4.0, 1e30], dtype=F)
SIZES = (1, 255, 257, 777, 1031)                       # the CPU premise; the GPU test uses its own list of n
IMAGES = ((37, 21), (16, 16), (4096, 4096))
ZERO_ROWS = 0.4                                        # share of rows whose gradient is all zero in a step


def _bounds(lo, hi):
    """Both bounds, the neighbour of each on the inside, -0.0."""
    lo, hi = F(lo), F(hi)
    return [lo, hi, np.nextafter(lo, hi), np.nextafter(hi, lo), F(-0.0)]


def param_choices(W, H):
    """Per field: the clamp bounds (main.cpp:741-749), their inward neighbours, -0.0, values outside, one inside."""
    pos_x = _bounds(0.0, W - 1) + [F(-5.0), F(W + 9), F(0.5 * (W - 1))]
    pos_y = _bounds(0.0, H - 1) + [F(-5.0), F(H + 9), F(-1e30), F(0.25 * (H - 1))]
    sigma = _bounds(1.0, 1024.0) + [F(0.25), F(5000.0), F(3.5)]
    rot = [F(-0.0), F(0.0), F(3e38), F(1e4), F(-0.7)]                   # not clamped
    colour = _bounds(0.0, 1.0) + [F(-1.0), F(2.0), F(0.5)]
    opacity = _bounds(0.1, 1.0) + [F(0.0), F(7.0), F(0.6)]
    return [np.array(c, dtype=F) for c in (pos_x, pos_y, sigma, sigma, rot, colour, colour, colour, opacity)]


def clamp_bounds(W, H):
    """(lo, hi) per field, None where the reference does not clamp (rot)."""
    return [(F(0), F(W) - F(1)), (F(0), F(H) - F(1)), (F(1), F(1024)), (F(1), F(1024)), None,
            (F(0), F(1)), (F(0), F(1)), (F(0), F(1)), (F(0.1), F(1))]


class Table:
    """splats (n, 9), adams (n, 9, 2), grads (steps, n, 9): contiguous float32."""

    def __init__(self, splats, adams, grads, W, H):
        self.splats, self.adams, self.grads, self.W, self.H = splats, adams, grads, W, H
        self.n = splats.shape[0]


def finite_table(n, W, H, steps=6, seed=0):
    rng = np.random.default_rng([n, W, H, steps, seed])
    choices = param_choices(W, H)
    splats = np.stack([c[rng.integers(0, len(c), n)] for c in choices], axis=1)
    adams = np.stack([FIRST_MOMENTS[rng.integers(0, len(FIRST_MOMENTS), (n, 9))],
                      SECOND_MOMENTS[rng.integers(0, len(SECOND_MOMENTS), (n, 9))]], axis=2)
    grads = GRADS[rng.integers(0, len(GRADS), (steps, n, 9))]
    # three rows in ten sleep through every step, one more in ten through each single step; in the first step a row
    # with an all-zero gradient has all-zero moments too (the state the dormant-block skip is about)
    sleepy = rng.random(n) < 0.3
    for s in range(steps):
        zero = sleepy | (rng.random(n) < (ZERO_ROWS - 0.3) / 0.7)
        grads[s, zero] = 0.0
        if s == 0:
            adams[zero] = 0.0
    return Table(np.ascontiguousarray(splats, dtype=F), np.ascontiguousarray(adams, dtype=F),
                 np.ascontiguousarray(grads, dtype=F), W, H)


# ---- overflow: finite inputs whose single step reaches inf / inf ------------------------------------------------------
OVERFLOW_ROWS = (256, 261, 299)


def overflow_table(fields, n=300, W=37, H=21):
    """+-FLT_MAX gradients and first moments with a second moment of 1e30 in `fields` of three rows past the first block:
    g * g is infinite, m / (1 - beta1t) is infinite, the quotient is NaN."""
    t = finite_table(n, W, H, steps=1, seed=7)
    for j, row in enumerate(OVERFLOW_ROWS):
        sign = F(-1.0) if j == 1 else F(1.0)
        for k in fields:
            t.grads[0, row, k] = sign * FLT_MAX
            t.adams[row, k] = (sign * FLT_MAX, F(1e30))
    return t


OVERFLOW_CASES = (("guarded fields", GUARDED, 1), ("every field", tuple(range(9)), 1), ("pos.y and opacity", (1, 8), 0))

# ---- non-finite gradients: nine fields x (+inf, -inf, NaN), one row each ----------------------------------------------
NONFINITE_ROW = 273                                    # in the second block of 256
NONFINITE_VALUES = (("+inf", F(np.inf)), ("-inf", F(-np.inf)), ("nan", F(np.nan)))
NONFINITE_CASES = tuple((k, name) for k in range(9) for name, _ in NONFINITE_VALUES)


def nonfinite_table(field, name, n=300, W=37, H=21):
    t = finite_table(n, W, H, steps=1, seed=11)
    t.grads[0, NONFINITE_ROW, field] = dict(NONFINITE_VALUES)[name]
    return t


def nonfinite_status(field):
    """What the reference does: abort for a guarded field, carry on with a NaN stored for pos.y and opacity."""
    return 1 if field in GUARDED else 0


# ---- dormant blocks ----------------------------------------------------------------------------------------------------
DORMANT_N = 3 * 256 + 5
DORMANT_ROWS = slice(256, 512)
DORMANT_WAKE = (3, 300, 2, DENORM_1)                   # step (0-based), row, field, gradient
DORMANT_WAKE_NEGATIVE = (4, 301, 0, F(-7.5))           # ... and a step later a row whose only gradient is negative
DORMANT_LAYOUTS = (1, 2, 3)


def _signed_zeros(rng, shape):
    return np.where(rng.random(shape) < 0.5, F(0.0), F(-0.0)).astype(F)


def dormant_table(layout, W=37, H=21, steps=5):
    """Rows 256..511 -- one whole block of the launch -- with zero gradients and zero moments around live blocks.
    layout 1: +0 and -0 mixed in both, anew in every step, and in step 4 a gradient of one denormal unit for row 300.
              The reference does not leave these rows alone (a -0.0 moment under a +0 gradient becomes +0), and a kernel
              that takes zero to mean +0 never skips this block: its -0.0 gradients and moments keep it running.
    layout 2: -0.0 gradients against +0 moments throughout.
    layout 3: +0 moments and +0 gradients only, so that after the first step the block really is asleep: three such steps,
              then in step 4 row 300 alone gets a gradient of one denormal unit (it rounds away in both moments, so the
              block is +0 again afterwards and only the zeroed gradient shows that it ran), and in step 5 row 301 alone
              gets -7.5.  tests/test_adam_edge_tables_cpu.py asserts the all-+0 premise before either wake-up."""
    t = finite_table(DORMANT_N, W, H, steps=steps, seed=20 + layout)
    rng = np.random.default_rng(layout)
    rows = DORMANT_ROWS
    if layout == 1:
        t.adams[rows] = _signed_zeros(rng, t.adams[rows].shape)
        for s in range(steps):
            t.grads[s, rows] = _signed_zeros(rng, t.grads[s, rows].shape)
        s, row, k, g = DORMANT_WAKE
        t.grads[s, row, k] = g
    elif layout == 2:
        t.adams[rows] = 0.0
        t.grads[:, rows] = F(-0.0)
    else:
        t.adams[rows] = 0.0
        t.grads[:, rows] = 0.0
        for s, row, k, g in (DORMANT_WAKE, DORMANT_WAKE_NEGATIVE):
            t.grads[s, row, k] = g
    return t


# ---- beta powers, as handed to s2d_set_adam ---------------------------------------------------------------------------
def beta_powers(k):
    """beta1t, beta2t after k iterations (main.cpp:718-719: one fp32 multiplication each per iteration)."""
    b1, b2 = F(1.0), F(1.0)
    for _ in range(k):
        b1, b2 = F(b1 * BETA1), F(b2 * BETA2)
    return b1, b2


# after 1200 multiplications: beta1t sits at four denormal units (4 * 0.9 = 3.6 rounds back to 4), beta2t = 5.78e-6
BETA_1200 = (np.array([4], dtype=np.uint32).view(F)[0], np.array([0x36C21561], dtype=np.uint32).view(F)[0])
BETAS = ((F(1.0), F(1.0), 0), (BETA_1200[0], BETA_1200[1], 1200), (F(0.0), F(0.0), 5000), (F(0.9), F(0.99), 1))


# ---- comparison --------------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def assert_same_bits(got, want, what=""):
    """NaN exactly where the other side has NaN; every other scalar with identical bits (-0 is not +0)."""
    got, want = np.ascontiguousarray(got, dtype=F), np.ascontiguousarray(want, dtype=F)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    if (gn != wn).any():
        at = np.argwhere(gn != wn)[0]
        raise AssertionError("%s: NaN on one side only at %s: got %r, want %r" % (what, tuple(at), got[tuple(at)], want[tuple(at)]))
    diff = (bits(got) != bits(want)) & ~wn
    if diff.any():
        at = tuple(np.argwhere(diff)[0])
        raise AssertionError("%s: %d scalars differ, first at %s: got %r (0x%08x), want %r (0x%08x)"
                             % (what, int(diff.sum()), at, got[at], bits(got)[at], want[at], bits(want)[at]))


# ---- the oracle's side -------------------------------------------------------------------------------------------------
class OracleState:
    """splats / adams / beta powers / iterations as main() holds them, stepped by s2do_adam_step on given gradients."""

    def __init__(self, splats, adams, W, H, beta1t=1.0, beta2t=1.0, iterations=0, fp32=False):
        self.splats = np.array(splats, dtype=F).reshape(-1, 9)
        self.adams = np.array(adams, dtype=F).reshape(-1, 9, 2)
        self.n, self.W, self.H, self.fp32 = self.splats.shape[0], W, H, bool(fp32)
        self.beta1t, self.beta2t = np.array([beta1t], dtype=F), np.array([beta2t], dtype=F)
        self.iterations = int(iterations)

    def step(self, grads, optimize_opacity):
        g = np.ascontiguousarray(grads, dtype=F).reshape(self.n, 9)
        L = O.lib()
        try:
            L.s2do_set_adam_fp32(1 if self.fp32 else 0)
            st = L.s2do_adam_step(O._p(self.splats), O._p(self.adams), O._p(g), self.n, self.W, self.H,
                                  O._p(self.beta1t), O._p(self.beta2t), int(bool(optimize_opacity)), float(LR))
        finally:
            L.s2do_set_adam_fp32(0)
        self.iterations += 1
        return st

    def copy(self):
        return OracleState(self.splats, self.adams, self.W, self.H, self.beta1t[0], self.beta2t[0], self.iterations, self.fp32)
