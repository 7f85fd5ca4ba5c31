"""Host replay of mgn_rollout with MGN_SOLVER_TSIT5_FIXED (a helper of the tests, not a test): `solve(prob, Tsit5(); adaptive = false, dt,
saveat = saves)` over ode_func_eval, the library's loop written out in NumPy float32 with the right-hand side as a callable (the tests
pass Engine.ode_step in its resident form, so every right-hand side is the device's own).

    grid and saves: tsit5_dense_ref.fixed_dense_steps / dense_plan (the rule include/mgn_hip.h states for step mode 2)
    evaluation form: the state, every stage input and x_{n+1} take, IN PLACE, the inflow rows of the frame of the time their stage sees
    (frame rule: solver_adjoint_ref.frame_of); save 0 is x0 before the first right-hand side

The stage sums are float32 products and additions in NumPy's order, where the device runs one fmaf chain per element: that rounding is
the only difference between the two, and the tests measure it on a run without an inflow mask before they use it as a tolerance."""
import numpy as np

import solver_adjoint_ref as sar
import tsit5_dense_ref as tdr
from mgn_amd.reference_api import TSIT5_A, TSIT5_C
from tsit5_adjoint_ref import _tt

F32 = np.float32


def _comb(u, h, coef, ks):
    s = np.zeros_like(u)
    for c, k in zip(coef, ks):
        s = s + F32(c) * k
    return (u + F32(h) * s).astype(F32)


def replay(rhs, x0, t0, t1, dt, saves_dt, n_saves, inflow_mask=None, inflow_data=None, time_type=F32, inflow_rule="reference"):
    """Returns (pred [n_saves][N][O] float32, step_t, step_h, plan, stats) -- plan as tsit5_dense_ref.dense_plan's, stats the counters
    mgn_rollout returns."""
    tt = _tt(time_type)
    sdt = tt(saves_dt)
    step_t, step_h, t_end = tdr.fixed_dense_steps(t0, t1, dt, saves_dt, time_type)
    plan = tdr.dense_plan(step_t, step_h, t_end, t0, saves_dt, n_saves, time_type)
    times = list(step_t) + [t_end]
    im = None if inflow_mask is None else np.asarray(inflow_mask).reshape(-1).astype(bool)

    def overwrite(x, t):
        if im is not None:
            x[im] = inflow_data[sar.frame_of(t, sdt, tt, len(inflow_data), inflow_rule)][im]
        return x

    u = np.array(x0, F32, copy=True)
    pred = [None] * n_saves
    pred[0] = u.copy()
    n_rhs = 1
    k1 = np.asarray(rhs(overwrite(u, times[0])), F32)
    for n, (t, h) in enumerate(zip(step_t, step_h)):
        k = [k1]
        for i in range(1, 6):
            y = overwrite(_comb(u, h, TSIT5_A[i][:i], k), tt(t + tt(TSIT5_C[i] * h)))
            k.append(np.asarray(rhs(y), F32))
        unew = overwrite(_comb(u, h, TSIT5_A[6], k), times[n + 1])
        k.append(np.asarray(rhs(unew), F32))
        n_rhs += 6
        for s, (idx, theta, hit) in enumerate(plan):
            if not hit and idx == n:
                pred[s] = _comb(u, h, tdr.interp_weights(theta), k)
        u, k1 = unew, k[6]
        for s, (idx, _, hit) in enumerate(plan):
            if hit and idx == n + 1:
                pred[s] = u.copy()
    for s, (idx, _, hit) in enumerate(plan):      # (no step at all: every save is x0)
        if pred[s] is None:
            assert hit and idx == len(step_h)
            pred[s] = u.copy()
    return np.stack(pred), step_t, step_h, plan, dict(n_accept=len(step_h), n_reject=0, n_rhs=n_rhs)
