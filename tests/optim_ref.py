"""The oracle's side of the optimiser controls (s2d_set_optim / s2d_set_frozen): the COMPOSITE oracle step.

The oracle's nine scalar Adam updates of a splat are independent (oracle/s2d_oracle.c, s2do_adam_step; main.cpp:721-738), so
a step with a rate per parameter group is put together from whole oracle steps: one s2do_adam_step per DISTINCT rate, each on
a copy of the state with its own beta words; the columns of a group taken from the call made at that group's rate; the rows of
frozen splats put back as they were.  Status 1 iff a guarded field (adam_cases.GUARDED) of a merged, unfrozen row is
non-finite -- the finite guard looks at what the step wrote, and it wrote nothing of a frozen row.

The rates are handed in as float32 -- in the GPU tests the library's own rounded values, Trainer.rates_at(), so that no
comparison depends on whose pow() rounds how.
"""
import numpy as np

import adam_cases as A
import oracle_lib as O

F = np.float32
GROUP_OF = (0, 0, 1, 1, 2, 3, 3, 3, 4)      # scalar k of a splat -> pos, scale, rot, colour, opacity
GROUP_COLUMNS = tuple([k for k in range(9) if GROUP_OF[k] == g] for g in range(5))
GAIN_RATES = (0.5, 0.2, 0.1, 0.05, 0.05)     # the constant rates of DESIGN.md section 15's table
TABLE_RATES = (0.5, 0.2, 0.1, 0.05, 0.05)    # the decaying configuration of the table tests:
TABLE_RATIOS = (0.1, 0.5, 1.0, 1.0, 0.25)    # ... the rate changes every step until T = 4, then stands
TABLE_T = 4


def rates_f64(rate, final_ratio, T, t):
    """The header's formula restated in float64 NumPy, rounded to float32 once (the CPU test's 1-ulp yardstick)."""
    out = np.zeros(5, dtype=F)
    for g in range(5):
        ratio = 1.0 if float(final_ratio[g]) == 0.0 else float(F(final_ratio[g]))
        if T == 0 or ratio == 1.0:
            out[g] = F(rate[g])
        else:
            out[g] = F(np.float64(F(rate[g])) * np.power(np.float64(ratio), np.float64(min(t, T)) / np.float64(T)))
    return out


def composite_step(splats, adams, grads, W, H, beta1t, beta2t, optimize_opacity, rates, frozen=None, fp32=False):
    """One step on float32 arrays (n, 9), (n, 9, 2), (n, 9) and one-element beta arrays, all updated IN PLACE.
    rates: five float32.  frozen: n booleans or None.  -> status."""
    n = splats.shape[0]
    rates = np.asarray(rates, dtype=F).reshape(5)
    g = np.ascontiguousarray(grads, dtype=F).reshape(n, 9)
    before_s, before_a = splats.copy(), adams.copy()
    L = O.lib()
    runs = {}
    try:
        L.s2do_set_adam_fp32(1 if fp32 else 0)
        for r in rates:
            key = int(A.bits(r).reshape(-1)[0])
            if key in runs:
                continue
            s, a, b1, b2 = before_s.copy(), before_a.copy(), beta1t.copy(), beta2t.copy()
            L.s2do_adam_step(O._p(s), O._p(a), O._p(g), n, W, H, O._p(b1), O._p(b2), int(bool(optimize_opacity)), float(r))
            runs[key] = (s, a, b1, b2)
    finally:
        L.s2do_set_adam_fp32(0)
    for grp in range(5):
        s, a, b1, b2 = runs[int(A.bits(rates[grp]).reshape(-1)[0])]
        cols = GROUP_COLUMNS[grp]
        splats[:, cols] = s[:, cols]
        adams[:, cols] = a[:, cols]
    beta1t[:], beta2t[:] = b1, b2          # (the same words in every run)
    live = np.ones(n, dtype=bool)
    if frozen is not None:
        fz = np.asarray(frozen).astype(bool)
        splats[fz], adams[fz] = before_s[fz], before_a[fz]
        live = ~fz
    bad = ~np.isfinite(splats[:, list(A.GUARDED)])
    return 1 if bad[live].any() else 0


class CompositeState(A.OracleState):
    """adam_cases.OracleState stepped by the composite oracle: step(grads, flag, rates, frozen)."""

    def step(self, grads, optimize_opacity, rates=None, frozen=None):
        if rates is None:
            rates = np.full(5, A.LR, dtype=F)
        st = composite_step(self.splats, self.adams, grads, self.W, self.H, self.beta1t, self.beta2t, optimize_opacity, rates,
                            frozen, self.fp32)
        self.iterations += 1
        return st

    def copy(self):
        return CompositeState(self.splats, self.adams, self.W, self.H, self.beta1t[0], self.beta2t[0], self.iterations, self.fp32)


def oracle_loop(target, n, iters, rates_of, frozen=None, optimize_opacity=False, splats=None):
    """The oracle's training loop (forward, backward, composite step) from init() (or `splats`); rates_of(t) -> five
    float32.  -> (OracleTrainer, [MSE printed for each iteration])."""
    o = O.OracleTrainer(target, n, optimize_opacity)
    if splats is not None:
        o.splats[:] = np.ascontiguousarray(splats).view(O.SPLAT_DTYPE).reshape(-1)
    trace = []
    for t in range(iters):
        o.forward()
        trace.append(o.mse())
        o.backward()
        sp = o.splats.view(F).reshape(n, 9)
        ad = o.adams.view(F).reshape(n, 9, 2)
        st = composite_step(sp, ad, o.dsplats.view(F).reshape(n, 9), o.W, o.H, o.beta1t, o.beta2t, optimize_opacity,
                            rates_of(t), frozen)
        assert st == 0, t
        o.iterations += 1
    return o, trace
