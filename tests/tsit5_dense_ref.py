"""Float64 reference driver of mgn_solver_grad_tsit5 with dense saves (a helper of the tests, not a test), the twin of
tsit5_adjoint_ref.py for MGN_TSIT5_DENSE_SAVES: `solve(prob, Tsit5(); saveat = saves)` without tstops over a GIVEN accepted step sequence,
and its discrete adjoint with the steps and the interpolation points held fixed.

    forward, per accepted step n (t_n, h_n) as tsit5_adjoint_ref, and k_{n,7} = f(z_{n+1,1}) (z_{n+1,1}: x_{n+1} with the inflow rows of
    frame(t_{n+1}); the same evaluation as k_{n+1,1});  a save strictly inside the step:
        xhat_s = x_n + h_n sum_{i=1..7} b_i(theta_s) k_{n,i},  theta_s = min((t_s - t_n) / h_n, 1),  b = interp_weights(theta_s)
    reverse, ghat_s = dL/dxhat_s, S_n the interpolated saves of step n:
        kbar_{n,i} = h_n (b_i lam + sum_{j>i} A[j][i] ybar_j) + h_n sum_{S_n} b_i(theta_s) ghat_s            (i = 1 .. 6)
        kbar_{n,1} also takes h_{n-1} sum_{S_{n-1}} b_7(theta_s) ghat_s;  S_{K-1}: one extra VJP at z_{K,1}, masked, added to lam_K
        lam_n = lam_{n+1} + sum_i ybar_i + sum_{S_n} ghat_s + dL/dx_n

The plan of the saves (dense_plan) is the library's rule: after step n every pending save time t_s <= t_{n+1} is taken; it is x_{n+1}
itself if |t_s - t_{n+1}| <= 1e-9 |t_{n+1}| + 1e-12, else interpolated; save 0 is x0; saves never reached are the final state."""
import numpy as np

import solver_adjoint_ref as sar
from mgn_amd.reference_api import TSIT5_A, TSIT5_C, TSIT5_R
from tsit5_adjoint_ref import _tt


def interp_weights(theta):
    th = float(theta)
    return np.array([sum(r[p] * th ** (p + 1) for p in range(4)) for r in TSIT5_R])


def dense_plan(step_t, step_h, t_end, t0, saves_dt, n_saves, time_type=np.float32):
    """[(index, theta, hit)] per save: hit -> the save is state `index` (theta None); else it is interpolated inside step `index`."""
    tt = _tt(time_type)
    times = [float(t) for t in step_t] + [float(t_end)]
    K = len(step_h)
    plan = [(0, None, True)]
    n = 0
    for s in range(1, n_saves):
        ts = tt(tt(t0) + s * tt(saves_dt))
        while n < K and ts > times[n + 1]:
            n += 1
        if n == K:
            plan.append((K, None, True))
        elif abs(ts - times[n + 1]) <= 1e-9 * abs(times[n + 1]) + 1e-12:
            plan.append((n + 1, None, True))
        else:
            plan.append((n, min((ts - times[n]) / float(step_h[n]), 1.0), False))
    return plan


def fixed_dense_steps(t0, t1, dt, saves_dt, time_type=np.float32):
    """(step_t, step_h, t_end) of the fixed-step mode with dense saves: t <- tt(t + dt) with h = dt; a step whose end lies within 1e-5
    saves_dt of t1 snaps onto it, one that would pass t1 is cut to tt(t1 - t)."""
    tt = _tt(time_type)
    t, t1, dt, sdt = tt(t0), tt(t1), tt(dt), tt(saves_dt)
    st, sh = [], []
    while t < t1 - 1e-5 * sdt:
        h, tn = dt, tt(t + dt)
        if abs(tn - t1) <= 1e-5 * sdt:
            tn = t1
        elif tn > t1:
            h, tn = tt(t1 - t), t1
        st.append(t)
        sh.append(h)
        t = tn
    return st, sh, t


def tsit5_dense_adjoint(rhs, vjp, x0, gt, step_t, step_h, t_end, plan, saves_dt, val_mask=None, inflow_mask=None, inflow_data=None,
                        loss_scale=None, cont_target=None, cont_weight=0.0, time_type=np.float32, inflow_rule="reference", rhs_at=None):
    """Returns (gs, loss, pred [n_saves][N][O], zs [K][6][N][O], dL/dx0).  rhs, vjp, rhs_at as tsit5_adjoint_ref.tsit5_adjoint's."""
    tt = _tt(time_type)
    sdt = tt(saves_dt)
    A = np.asarray(TSIT5_A, np.float64)
    x = np.asarray(x0, np.float64)
    N, O = x.shape
    K = len(step_h)
    n_saves = len(plan)
    gt = np.asarray(gt, np.float64)
    vm = np.ones((N, 1)) if val_mask is None else np.asarray(val_mask, np.float64).reshape(N, 1)
    ls = np.ones((1, O)) if loss_scale is None else np.asarray(loss_scale, np.float64).reshape(1, O)
    im = None if inflow_mask is None else np.asarray(inflow_mask).reshape(N).astype(bool)
    times = [float(t) for t in step_t] + [float(t_end)]

    def stage_input(y, t):
        if im is None:
            return y.copy(), None
        fr = sar.frame_of(t, sdt, tt, len(inflow_data), inflow_rule)
        z = y.copy()
        z[im] = np.asarray(inflow_data[fr], np.float64)[im]
        return z, fr

    def f(z, fr):
        return np.asarray(rhs_at(z, fr) if rhs_at is not None else rhs(z), np.float64)

    xs, zs, ks = [x], [], []
    z1, fr1 = stage_input(x, times[0]) if K else (None, None)
    k1 = f(z1, fr1) if K else None
    for n in range(K):
        t, h = times[n], float(step_h[n])
        k, z = [k1], [z1]
        for i in range(1, 6):
            zi, fr = stage_input(xs[-1] + h * sum(A[i][j] * k[j] for j in range(i)), tt(t + tt(TSIT5_C[i] * h)))
            z.append(zi)
            k.append(f(zi, fr))
        xs.append(xs[-1] + h * sum(A[6][j] * k[j] for j in range(6)))
        z1, fr1 = stage_input(xs[-1], times[n + 1])        # z_{n+1,1}: stage 7 of this step, stage 1 of the next
        k1 = f(z1, fr1)
        zs.append(z)
        ks.append(k + [k1])
    z_end = z1
    D = float(n_saves * N * O)
    pred, ghat = [], {}
    for s, (idx, theta, hit) in enumerate(plan):
        if hit:
            pred.append(xs[idx])
        else:
            b = interp_weights(theta)
            pred.append(xs[idx] + float(step_h[idx]) * sum(b[i] * ks[idx][i] for i in range(7)))
            ghat[s] = -2.0 * ls * ls * (gt[s] - pred[s]) * vm / D
    loss = sum(float((((gt[s] - pred[s]) * ls) ** 2 * vm).sum()) for s in range(n_saves)) / D
    ct = None if cont_target is None else np.asarray(cont_target, np.float64)
    if ct is not None:
        loss += float(cont_weight) * float(np.abs(xs[K] - ct).sum())

    def dl_dx(k):
        g = np.zeros((N, O))
        for s, (idx, _, hit) in enumerate(plan):
            if hit and idx == k:
                g += -2.0 * ls * ls * (gt[s] - xs[k]) * vm / D
        if k == K and ct is not None:
            g += float(cont_weight) * np.sign(xs[K] - ct)
        return g

    def sums(n):     # (sum ghat, W_1 .. W_7) of step n
        G, W = np.zeros((N, O)), [np.zeros((N, O)) for _ in range(7)]
        for s, (idx, theta, hit) in enumerate(plan):
            if not hit and idx == n:
                b = interp_weights(theta)
                G = G + ghat[s]
                W = [W[i] + b[i] * ghat[s] for i in range(7)]
        return G, W

    def masked(zb):
        zb = np.asarray(zb, np.float64).copy()
        if im is not None:
            zb[im] = 0.0
        return zb

    lam = dl_dx(K)
    gs = None
    if K and any(not hit and idx == K - 1 for idx, _, hit in plan):
        zb, g = vjp(z_end, float(step_h[K - 1]) * sums(K - 1)[1][6])
        lam = lam + masked(zb)
        gs = np.asarray(g, np.float64).copy()
    for n in range(K - 1, -1, -1):
        h, ybar = float(step_h[n]), [None] * 6
        G, W = sums(n)
        for i in range(5, -1, -1):
            kbar = h * (A[6][i] * lam + sum(A[j][i] * ybar[j] for j in range(i + 1, 6))) + h * W[i]
            if i == 0 and n > 0:
                kbar = kbar + float(step_h[n - 1]) * sums(n - 1)[1][6]
            zb, g = vjp(zs[n][i], kbar)
            ybar[i] = masked(zb)
            gs = np.asarray(g, np.float64).copy() if gs is None else gs + np.asarray(g, np.float64)
        lam = lam + sum(ybar) + G + dl_dx(n)
    return gs, loss, np.stack(pred), zs, lam
