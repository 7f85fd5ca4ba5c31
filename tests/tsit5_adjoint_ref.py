"""Float64 reference driver of mgn_solver_grad_tsit5 (a helper of the tests, not a test), the twin of solver_adjoint_ref.py: the loss of
one Tsit5 solve of ode_func_train (reference src/solve.jl:101-117) over a GIVEN accepted step sequence, and its discrete adjoint with
that sequence held fixed, written out stage by stage with the right-hand side and its VJP as callables.

    z_{n,i} = x_n + h_n sum_{j<i} A[i][j] k_{n,j}, the inflow rows of frame(t_{n,i}) written into a copy;  k_{n,i} = f(z_{n,i})
    t_{n,1} = t_n, t_{n,i} = tt(t_n + tt(c_i h_n));  x_{n+1} = x_n + h_n sum_i b_i k_{n,i}
    reverse: kbar_i = h_n (b_i lam + sum_{j>i} A[j][i] ybar_j);  (zbar_i, g_i) = VJP at z_{n,i};  ybar_i = zbar_i, inflow rows zeroed
             lam_n = lam_{n+1} + sum_i ybar_i + dL/dx_n;  gs = sum g

rhs(x) -> f(x) [N][O];  vjp(x, lam) -> (lam^T df/dx, lam^T df/dps)."""
import numpy as np

import solver_adjoint_ref as sar
from mgn_amd.reference_api import TSIT5_A, TSIT5_C


def _tt(time_type):
    f64 = np.dtype(time_type) == np.float64
    return (lambda v: float(v)) if f64 else (lambda v: float(np.float32(v)))


def fixed_steps(t0, t1, dt, saves_dt, n_saves, time_type=np.float32):
    """(step_t, step_h, save_step, t_end) of the fixed-step mode: solver_adjoint_ref.time_grid's Euler grid, h = dt every step."""
    ts, steps, _, tt = sar.time_grid(t0, t1, dt, saves_dt, n_saves, time_type)
    return ts[:-1], [tt(dt)] * (len(ts) - 1), steps, ts[-1]


def adaptive_saves(step_t, t_end, t0, saves_dt, n_saves, time_type=np.float32):
    """The state each save is under tstops = saves: the first state (times step_t, then t_end) that sits on the save's time; a save the
    solve stops short of (an ulp) is the final state."""
    tt = _tt(time_type)
    times = list(step_t) + [t_end]
    out = []
    for s in range(n_saves):
        ts = tt(tt(t0) + s * tt(saves_dt))
        hit = [n for n, t in enumerate(times) if abs(ts - t) <= 1e-9 * abs(t) + 1e-12]
        out.append(hit[0] if hit else len(times) - 1)
    return out


def tsit5_adjoint(rhs, vjp, x0, gt, step_t, step_h, save_step, saves_dt, val_mask=None, inflow_mask=None, inflow_data=None,
                  loss_scale=None, cont_target=None, cont_weight=0.0, time_type=np.float32, inflow_rule="reference", rhs_at=None):
    """Returns (gs, loss, pred [n_saves][N][O], zs [K][6][N][O] -- the arrays the stage right-hand sides saw).  rhs_at(x, fr): optional
    right-hand side that also receives the inflow frame index (for an oracle that overwrites the rows itself)."""
    tt = _tt(time_type)
    sdt = tt(saves_dt)
    A = np.asarray(TSIT5_A, np.float64)
    x = np.asarray(x0, np.float64)
    N, O = x.shape
    K = len(step_h)
    n_saves = len(save_step)
    gt = np.asarray(gt, np.float64)
    vm = np.ones((N, 1)) if val_mask is None else np.asarray(val_mask, np.float64).reshape(N, 1)
    ls = np.ones((1, O)) if loss_scale is None else np.asarray(loss_scale, np.float64).reshape(1, O)
    im = None if inflow_mask is None else np.asarray(inflow_mask).reshape(N).astype(bool)
    xs, zs = [x], []
    for n in range(K):
        t, h = float(step_t[n]), float(step_h[n])
        k, z = [], []
        for i in range(6):
            zi = xs[-1] + h * sum(A[i][j] * k[j] for j in range(i)) if i else xs[-1].copy()
            fr = None
            if im is not None:
                ti = t if i == 0 else tt(t + tt(TSIT5_C[i] * h))
                fr = sar.frame_of(ti, sdt, tt, len(inflow_data), inflow_rule)
                zi = zi.copy()
                zi[im] = np.asarray(inflow_data[fr], np.float64)[im]
            z.append(zi)
            k.append(np.asarray(rhs_at(zi, fr) if rhs_at is not None else rhs(zi), np.float64))
        zs.append(z)
        xs.append(xs[-1] + h * sum(A[6][j] * k[j] for j in range(6)))
    D = float(n_saves * N * O)
    loss = sum(float((((gt[s] - xs[save_step[s]]) * ls) ** 2 * vm).sum()) for s in range(n_saves)) / D
    ct = None if cont_target is None else np.asarray(cont_target, np.float64)
    if ct is not None:
        loss += float(cont_weight) * float(np.abs(xs[K] - ct).sum())

    def dl_dx(k):
        g = np.zeros((N, O))
        for s in range(n_saves):
            if save_step[s] == k:
                g += -2.0 * ls * ls * (gt[s] - xs[k]) * vm / D
        if k == K and ct is not None:
            g += float(cont_weight) * np.sign(xs[K] - ct)
        return g

    lam = dl_dx(K)
    gs = None
    for n in range(K - 1, -1, -1):
        h, ybar = float(step_h[n]), [None] * 6
        for i in range(5, -1, -1):
            kbar = h * (A[6][i] * lam + sum(A[j][i] * ybar[j] for j in range(i + 1, 6)))
            zb, g = vjp(zs[n][i], kbar)
            zb = np.asarray(zb, np.float64).copy()
            if im is not None:
                zb[im] = 0.0
            ybar[i] = zb
            gs = np.asarray(g, np.float64).copy() if gs is None else gs + np.asarray(g, np.float64)
        lam = lam + sum(ybar) + dl_dx(n)
    pred = np.stack([xs[save_step[s]] for s in range(n_saves)])
    return gs, loss, pred, zs
