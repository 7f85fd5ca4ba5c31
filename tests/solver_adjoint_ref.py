"""Float64 reference driver of mgn_solver_grad (a helper of the tests, not a test): the loss of one fixed-step Euler solve of
ode_func_train (reference src/solve.jl:101-117, strategies.jl:175-196, 257-292, 365-378) and its discrete adjoint, written out step by
step with the right-hand side and its VJP as callables -- like reference_api.solver_training_euler, plus the inflow copy, the save
rule and time grid of the native Euler loop, loss_scale and the continuity (L1) term.

    x_{k+1} = x_k + dt f(P_k x_k)          P_k: the inflow rows of frame floor(t_k / saves_dt) written into a copy
    loss    = sum_s ((ls (gt_s - x_{k_s}))^2 vm) / (n_saves N O) + cw sum |x_K - ct|
    a_K     = dL/dx_K;   a_k = dL/dx_k + a_{k+1} + (1 - inflow) .* J_x f(P_k x_k)^T (dt a_{k+1});   gs = sum_k J_p f(P_k x_k)^T (dt a_{k+1})

rhs(x) -> f(x) [N][O];  vjp(x, lam) -> (lam^T df/dx, lam^T df/dps)."""
import numpy as np


def time_grid(t0, t1, dt, saves_dt, n_saves, time_type=np.float32):
    """(times t_k of the K + 1 states, the step of every save), as the native Euler loop walks them: t <- t + dt in the time type,
    the last step snapped onto t1, a save at the step whose end lies within dt / 4 past its point.  Raises if a save is not reached."""
    f64 = np.dtype(time_type) == np.float64

    def tt(v):
        return float(v) if f64 else float(np.float32(v))

    t0, t1, dt, sdt = tt(t0), tt(t1), tt(dt), tt(saves_dt)
    K = int(round((t1 - t0) / dt))
    ts, steps = [t0], [0]
    t = t0
    for i in range(K):
        t = t1 if (i + 1 == K and abs(tt(t + dt) - t1) <= 1e-5 * sdt) else tt(t + dt)
        ts.append(t)
        while len(steps) < n_saves and tt(t0 + len(steps) * sdt) <= t + 0.25 * dt:
            steps.append(i + 1)
    if len(steps) < n_saves:
        raise ValueError("a save point lies beyond the end of the solve")
    return ts, steps, sdt, tt


def frame_of(t, sdt, tt, n_frames, inflow_rule="reference"):
    if inflow_rule == "tolerant":
        return min(max(int(np.floor(t / sdt + 1e-3)), 0), n_frames - 1)
    fr = int(np.floor(tt(t / sdt)))
    if fr < 0 or fr >= n_frames:
        raise IndexError(f"inflow frame {fr} at t = {t} (BoundsError)")
    return fr


def euler_adjoint(rhs, vjp, x0, gt, t0, t1, dt, saves_dt, n_saves, val_mask=None, inflow_mask=None, inflow_data=None, loss_scale=None,
                  cont_target=None, cont_weight=0.0, time_type=np.float32, inflow_rule="reference", rhs_at=None):
    """Returns (gs, loss, pred [n_saves][N][O], xin [K][N][O] -- the arrays the right-hand sides saw).  rhs_at(x, fr): optional
    right-hand side that also receives the inflow frame index (for an oracle that overwrites the rows itself)."""
    ts, steps, sdt, tt = time_grid(t0, t1, dt, saves_dt, n_saves, time_type)
    dtv = tt(dt)
    K = len(ts) - 1
    x = np.asarray(x0, np.float64)
    N, O = x.shape
    gt = np.asarray(gt, np.float64)
    vm = np.ones((N, 1)) if val_mask is None else np.asarray(val_mask, np.float64).reshape(N, 1)
    ls = np.ones((1, O)) if loss_scale is None else np.asarray(loss_scale, np.float64).reshape(1, O)
    im = None if inflow_mask is None else np.asarray(inflow_mask).reshape(N).astype(bool)
    xs, xin = [x], []
    for k in range(K):
        xk = xs[-1].copy()
        fr = None
        if im is not None:
            fr = frame_of(ts[k], sdt, tt, len(inflow_data), inflow_rule)
            xk[im] = np.asarray(inflow_data[fr], np.float64)[im]
        xin.append(xk)
        f = rhs_at(xk, fr) if rhs_at is not None else rhs(xk)
        xs.append(xs[-1] + dtv * np.asarray(f, np.float64))
    D = float(n_saves * N * O)
    loss = sum(float((((gt[s] - xs[steps[s]]) * ls) ** 2 * vm).sum()) for s in range(n_saves)) / D
    ct = None if cont_target is None else np.asarray(cont_target, np.float64)
    if ct is not None:
        loss += float(cont_weight) * float(np.abs(xs[K] - ct).sum())

    def dl_dx(k):
        g = np.zeros((N, O))
        for s in range(n_saves):
            if steps[s] == k:
                g += -2.0 * ls * ls * (gt[s] - xs[k]) * vm / D
        if k == K and ct is not None:
            g += float(cont_weight) * np.sign(xs[K] - ct)
        return g

    a = dl_dx(K)
    gs = None
    for k in range(K - 1, -1, -1):
        xbar, g = vjp(xin[k], dtv * a)
        xbar = np.asarray(xbar, np.float64)
        if im is not None:
            xbar = xbar.copy()
            xbar[im] = 0.0
        gs = np.asarray(g, np.float64).copy() if gs is None else gs + np.asarray(g, np.float64)
        a = dl_dx(k) + a + xbar
    pred = np.stack([xs[steps[s]] for s in range(n_saves)])
    return gs, loss, pred, xin
