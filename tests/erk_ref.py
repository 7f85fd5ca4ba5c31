"""Host references of the *_erk entry points (a helper of the tests, not a test), generic in the tableau (an ErkTableau, or anything
with its stages / fsal / A / b / c):

replay: mgn_rollout_erk with adaptive = 0 -- `solve(prob, alg; adaptive = false, dt, saveat = saves)` over ode_func_eval -- written out
    in NumPy float32 with the right-hand side as a callable (the tests pass Engine.ode_step in its resident form, so every right-hand
    side is the device's own), modelled on tsit5_fixed_eval_ref.py.  Grid and save plan: solver_adjoint_ref.time_grid.  Evaluation
    form: every right-hand side overwrites, IN PLACE, the inflow rows of the array it is evaluated on with the frame of the time its
    stage sees; the FSAL stage is evaluated on x_{n+1} at t_{n+1}; without FSAL x_{n+1} is saved as the update left it and stage 1 of
    the next step overwrites it.  Terms whose coefficient is exactly 0 are left out.  The stage sums are float32 products and additions
    in NumPy's order, where the device runs one fmaf chain per element: that rounding is the only difference between the two.

erk_adjoint: the float64 loss of one fixed-step solve of ode_func_train with the tableau and its discrete adjoint, modelled on
    tsit5_adjoint_ref.py: the s' = s - fsal active stages, x_{n+1} = x_n + h sum_i b_i k_{n,i}."""
import numpy as np

import solver_adjoint_ref as sar

F32 = np.float32


def _comb(u, h, coef, ks):
    s = np.zeros_like(u)
    for c, k in zip(coef, ks):
        if c != 0.0:
            s = s + F32(c) * k
    return (u + F32(h) * s).astype(F32)


def replay(rhs, tab, x0, t0, t1, dt, saves_dt, n_saves, inflow_mask=None, inflow_data=None, time_type=F32, inflow_rule="reference"):
    """Returns (pred [n_saves][N][O] float32, stats: the counters mgn_rollout_erk returns)."""
    ts, steps, sdt, tt = sar.time_grid(t0, t1, dt, saves_dt, n_saves, time_type)
    K, h = len(ts) - 1, tt(dt)
    A, b, c, s, fsal = np.asarray(tab.A), np.asarray(tab.b), np.asarray(tab.c), int(tab.stages), bool(tab.fsal)
    im = None if inflow_mask is None else np.asarray(inflow_mask).reshape(-1).astype(bool)

    def f(x, t):      # the in-place overwrite, then the right-hand side
        if im is not None:
            x[im] = inflow_data[sar.frame_of(t, sdt, tt, len(inflow_data), inflow_rule)][im]
        return np.asarray(rhs(x), F32)

    u = np.array(x0, F32, copy=True)
    pred = [u.copy() for q in range(n_saves) if steps[q] == 0]
    n_rhs = 0
    k1 = None
    if fsal:
        k1, n_rhs = f(u, ts[0]), 1
    for n in range(K):
        t = ts[n]
        if not fsal:
            k1, n_rhs = f(u, t), n_rhs + 1
        k = [k1]
        for i in range(1, s - 1 if fsal else s):
            y = _comb(u, h, A[i, :i], k)
            k.append(f(y, tt(t + tt(c[i] * h))))
            n_rhs += 1
        if fsal:
            unew = _comb(u, h, A[s - 1, :s - 1], k)
            k1, n_rhs = f(unew, ts[n + 1]), n_rhs + 1
        else:
            unew = _comb(u, h, b, k)
        u = unew
        pred += [u.copy() for q in range(n_saves) if steps[q] == n + 1]
    return np.stack(pred), dict(n_accept=K, n_reject=0, n_rhs=n_rhs)


def erk_adjoint(rhs, vjp, tab, x0, gt, t0, t1, dt, saves_dt, n_saves, val_mask=None, inflow_mask=None, inflow_data=None, loss_scale=None,
                cont_target=None, cont_weight=0.0, time_type=F32, inflow_rule="reference", rhs_at=None):
    """Returns (gs, loss, pred [n_saves][N][O]) in float64.  rhs(x) -> f(x) [N][O];  vjp(x, lam) -> (lam^T df/dx, lam^T df/dps);
    rhs_at(x, fr): optional right-hand side that also receives the inflow frame index."""
    ts, save_step, sdt, tt = sar.time_grid(t0, t1, dt, saves_dt, n_saves, time_type)
    K, h = len(ts) - 1, tt(dt)
    A, b, c = np.asarray(tab.A, np.float64), np.asarray(tab.b, np.float64), np.asarray(tab.c, np.float64)
    sp = int(tab.stages) - (1 if tab.fsal else 0)
    x = np.asarray(x0, np.float64)
    N, O = x.shape
    gt = np.asarray(gt, np.float64)
    vm = np.ones((N, 1)) if val_mask is None else np.asarray(val_mask, np.float64).reshape(N, 1)
    ls = np.ones((1, O)) if loss_scale is None else np.asarray(loss_scale, np.float64).reshape(1, O)
    im = None if inflow_mask is None else np.asarray(inflow_mask).reshape(N).astype(bool)
    xs, zs = [x], []
    for n in range(K):
        t = ts[n]
        k, z = [], []
        for i in range(sp):
            zi = xs[-1] + h * sum(A[i][j] * k[j] for j in range(i)) if i else xs[-1].copy()
            fr = None
            if im is not None:
                fr = sar.frame_of(t if i == 0 else tt(t + tt(c[i] * h)), sdt, tt, len(inflow_data), inflow_rule)
                zi = zi.copy()
                zi[im] = np.asarray(inflow_data[fr], np.float64)[im]
            z.append(zi)
            k.append(np.asarray(rhs_at(zi, fr) if rhs_at is not None else rhs(zi), np.float64))
        zs.append(z)
        xs.append(xs[-1] + h * sum(b[j] * k[j] for j in range(sp)))
    D = float(n_saves * N * O)
    loss = sum(float((((gt[q] - xs[save_step[q]]) * ls) ** 2 * vm).sum()) for q in range(n_saves)) / D
    ct = None if cont_target is None else np.asarray(cont_target, np.float64)
    if ct is not None:
        loss += float(cont_weight) * float(np.abs(xs[K] - ct).sum())

    def dl_dx(k):
        g = np.zeros((N, O))
        for q in range(n_saves):
            if save_step[q] == k:
                g += -2.0 * ls * ls * (gt[q] - xs[k]) * vm / D
        if k == K and ct is not None:
            g += float(cont_weight) * np.sign(xs[K] - ct)
        return g

    lam = dl_dx(K)
    gs = None
    for n in range(K - 1, -1, -1):
        ybar = [None] * sp
        for i in range(sp - 1, -1, -1):
            kbar = h * (b[i] * lam + sum(A[j][i] * ybar[j] for j in range(i + 1, sp)))
            zb, g = vjp(zs[n][i], kbar)
            zb = np.asarray(zb, np.float64).copy()
            if im is not None:
                zb[im] = 0.0
            ybar[i] = zb
            gs = np.asarray(g, np.float64).copy() if gs is None else gs + np.asarray(g, np.float64)
        lam = lam + sum(ybar) + dl_dx(n)
    pred = np.stack([xs[save_step[q]] for q in range(n_saves)])
    return gs, loss, pred
