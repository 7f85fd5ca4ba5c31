"""mgn_shooting_grad (Engine.shooting_grad, train_step_multiple_shooting(batched=True)): all MultipleShooting windows in one call,
against the per-window loop of mgn_solver_grad / mgn_solver_grad_tsit5 and against the float64 driver of tests/solver_adjoint_ref.py.
Run on the MI355X box with `-m gpu`."""
import numpy as np
import pytest
import torch   # before the engine's first HIP call (device-array test), or torch finds no GPU afterwards

import solver_adjoint_ref as sar
from mgn_amd import MgnError, _capi
from mgn_amd import reference_api as ra
from test_gpu_solver_train import oracle_fns, problem, rel_l2
from util import cfg_dict, engine_for, make_params, rel_max, renumbered

pytestmark = pytest.mark.gpu

DT = 0.01


def tstop_of(T):
    return round((T - 1) * DT, 10)


def loop_and_batched(P, T, interval, solver="Euler", cw=0.3, **kw):
    eng, gt = P["eng"], P["gt"][:T]
    args = (eng, gt, P["onehot"], P["ef_raw"], 0.0, DT, tstop_of(T), interval, cw)
    common = dict(val_mask=P["vm"], solver=solver, adaptive=False, **kw)
    gs_l, loss_l = ra.train_step_multiple_shooting(*args, **common)
    gs_b, loss_b = ra.train_step_multiple_shooting(*args, batched=True, **common)
    return gs_l, loss_l, gs_b, loss_b


def window_preds(P, T, interval, solver="Euler", cw=0.3, time_type=np.float32, **kw):
    """Every window's predicted saves from the single-window calls, in window order."""
    eng, gt = P["eng"], P["gt"]
    ranges = ra.multiple_shooting_ranges(T, interval)
    out = []
    for i, (a, b) in enumerate(ranges):
        t0, t1 = ra._range_at(0.0, DT, a, time_type), ra._range_at(0.0, DT, b, time_type)
        ct = gt[ranges[i + 1][0]] if i + 1 < len(ranges) else None
        w = dict(val_mask=P["vm"], cont_target=ct, cont_weight=cw if ct is not None else 0.0, time_type=time_type, **kw)
        if solver == "Euler":
            _, _, pred = eng.solver_grad(gt[a], P["onehot"], P["ef_raw"], gt[a:b + 1], t0, t1, DT, DT, b - a + 1, want_pred=True, **w)
        else:
            pred = eng.solver_grad_tsit5(gt[a], P["onehot"], P["ef_raw"], gt[a:b + 1], t0, t1, DT, b - a + 1, dt=DT, adaptive=False,
                                         want_pred=True, **w)[2]["pred"]
        out.append(pred)
    return np.concatenate(out)


def batched(P, T, interval, solver="Euler", cw=0.3, time_type=np.float32, want_pred=True, **kw):
    eng, gt = P["eng"], P["gt"]
    ranges = ra.multiple_shooting_ranges(T, interval)
    return eng.shooting_grad(P["onehot"], P["ef_raw"], gt, ranges, [ra._range_at(0.0, DT, a, time_type) for a, _ in ranges],
                             [ra._range_at(0.0, DT, b, time_type) for _, b in ranges], DT, DT, val_mask=P["vm"], cont_weight=cw,
                             time_type=time_type, solver=solver, want_pred=want_pred, **kw)


@pytest.mark.parametrize("solver", ["Euler", "Tsit5"])
def test_batched_matches_the_window_loop(solver):
    T, interval = 8, 4                                   # windows (0, 3), (3, 6), (6, 7): two step plans
    P = problem(K=T - 1)
    gs_l, loss_l, gs_b, loss_b = loop_and_batched(P, T, interval, solver=solver)
    assert abs(loss_b - loss_l) <= 1e-5 * abs(loss_l), (loss_b, loss_l)
    assert rel_l2(gs_b, gs_l) <= 1e-4, rel_l2(gs_b, gs_l)
    _, loss, pred = batched(P, T, interval, solver=solver)
    st = P["eng"].last_shooting
    assert st["n_groups"] == 2 and st["n_passes"] == 2, st
    assert abs(loss - loss_b) <= 1e-6 * abs(loss_b)
    ref = window_preds(P, T, interval, solver=solver)
    assert pred.shape == ref.shape
    assert rel_max(pred, ref) <= 1e-4, rel_max(pred, ref)


@pytest.mark.parametrize("time_type", [np.float32, np.float64])
def test_windows_read_their_own_inflow_frames(time_type):
    T, interval = 8, 4
    P = problem(K=T - 1)
    gt, N = P["gt"], P["N"]
    im = (P["node_type"] == 4) | (P["node_type"] == 1)
    assert im.any()
    frames = (gt[0][None] * (1.0 + 0.5 * P["rng"].standard_normal((T, N, 2)))
              + 0.5 * P["rng"].standard_normal((T, N, 2))).astype(np.float32)      # a different frame every step
    kw = dict(inflow_mask=im.astype(np.uint8), inflow_data=frames)
    gs, loss = batched(P, T, interval, time_type=time_type, want_pred=False, **kw)
    o_rhs, o_vjp, o_rhs_at = oracle_fns(P, inflow_mask=im, frames=frames)
    ranges = ra.multiple_shooting_ranges(T, interval)
    gs_o, loss_o = 0.0, 0.0
    for i, (a, b) in enumerate(ranges):
        ct = gt[ranges[i + 1][0]] if i + 1 < len(ranges) else None
        g, l, _, _ = sar.euler_adjoint(o_rhs, o_vjp, gt[a], gt[a:b + 1], ra._range_at(0.0, DT, a, time_type), ra._range_at(0.0, DT, b, time_type),
                                       DT, DT, b - a + 1, val_mask=P["vm"], cont_target=ct, cont_weight=0.3 if ct is not None else 0.0,
                                       time_type=time_type, inflow_rule="reference", rhs_at=o_rhs_at, **kw)
        gs_o, loss_o = gs_o + np.asarray(g, np.float64), loss_o + l
    assert abs(loss - loss_o) <= 1e-4 * abs(loss_o), (loss, loss_o)
    assert rel_l2(gs, gs_o) <= 5e-3, rel_l2(gs, gs_o)
    # the frames matter: the same windows with every window on frame 0 .. give another loss
    gs0, loss0 = batched(P, T, interval, time_type=time_type, want_pred=False, inflow_mask=im.astype(np.uint8),
                         inflow_data=np.repeat(frames[:1], T, axis=0))
    assert abs(loss0 - loss_o) > 1e-3 * abs(loss_o)


def test_pass_size():
    T, interval = 11, 4                                  # (0, 3), (3, 6), (6, 9), (9, 10): a group of three and the short last window
    P = problem(K=T - 1)
    res = {}
    for cap, passes in ((1, 4), (2, 3), (0, 2)):
        gs, loss, pred = batched(P, T, interval, max_windows_per_pass=cap)
        st = P["eng"].last_shooting
        assert st["n_groups"] == 2 and st["n_passes"] == passes, (cap, st)
        res[cap] = (gs.copy(), loss, pred)
    for cap in (2, 0):
        assert abs(res[cap][1] - res[1][1]) <= 1e-5 * abs(res[1][1])
        assert rel_l2(res[cap][0], res[1][0]) <= 1e-4
    assert np.array_equal(res[1][2], window_preds(P, T, interval))        # one window per pass: the single-window code, bit for bit


def test_handles_renumbered_device_tensors_and_graph_change():
    T, interval = 8, 4
    P = problem(K=T - 1, scramble=True, n_points=400)
    eng, gt = P["eng"], P["gt"]
    assert renumbered(eng)
    ranges = ra.multiple_shooting_ranges(T, interval)
    t0s, t1s = [a * DT for a, _ in ranges], [b * DT for _, b in ranges]
    dev = torch.device("cuda", 0)
    gt_t = torch.from_numpy(gt).to(dev)
    outs = [torch.full((eng.param_count,), float("nan"), dtype=torch.float32, device=dev) for _ in range(2)]
    torch.cuda.synchronize()
    single = dict(val_mask=P["vm"])
    g0, l0 = eng.solver_grad(gt[0], P["onehot"], P["ef_raw"], gt[:4], 0.0, 0.03, DT, DT, 4, **single)
    r0 = eng.rollout("Euler", gt[0], P["onehot"], P["ef_raw"], 0.0, 0.03, DT, 4, dt=DT, val_mask=P["vm"])[0]
    losses = []
    for o in outs:
        _, l = eng.shooting_grad(P["onehot"], P["ef_raw"], gt_t, ranges, t0s, t1s, DT, DT, val_mask=P["vm"], cont_weight=0.3, out=o)
        losses.append(l)
    torch.cuda.synchronize()
    assert losses[0] == losses[1] and torch.equal(outs[0], outs[1])                # bitwise repeatable
    gs_l, loss_l, _, _ = loop_and_batched(P, T, interval)
    assert abs(losses[0] - loss_l) <= 1e-5 * abs(loss_l)
    assert rel_l2(outs[0].cpu().numpy(), gs_l) <= 1e-4
    g1, l1 = eng.solver_grad(gt[0], P["onehot"], P["ef_raw"], gt[:4], 0.0, 0.03, DT, DT, 4, **single)
    r1 = eng.rollout("Euler", gt[0], P["onehot"], P["ef_raw"], 0.0, 0.03, DT, 4, dt=DT, val_mask=P["vm"])[0]
    assert l0 == l1 and np.array_equal(g0, g1) and np.array_equal(r0, r1)           # the handle's own calls are untouched
    # another mesh on the same handle: no stale companion graph
    Q = problem(K=T - 1, n_points=260, seed=9)
    eng.set_graph(Q["s"], Q["r"], Q["N"])
    Q["eng"].close()
    Q["eng"] = eng
    gs_l, loss_l, gs_b, loss_b = loop_and_batched(Q, T, interval)
    assert abs(loss_b - loss_l) <= 1e-5 * abs(loss_l), (loss_b, loss_l)
    assert rel_l2(gs_b, gs_l) <= 1e-4


def test_refusals_leave_the_handle_usable():
    T, interval = 8, 4
    P = problem(K=T - 1)
    eng = P["eng"]
    with pytest.raises(MgnError) as ei:
        batched(P, T, interval, solver="Tsit5", adaptive=True)
    assert ei.value.code == _capi.MGN_E_UNSUPPORTED
    _, loss_ok = batched(P, T, interval, want_pred=False)
    s, r, N = P["s"], P["r"], P["N"]
    two = engine_for(P["cfg"], Fe2=3)
    two.set_params(np.zeros(two.param_count, np.float32))
    two.set_graph(s, r, N)
    two.set_edge_set(1, r[:10], s[:10])
    two.set_edge_features(1, np.zeros((10, 3), np.float32))
    with pytest.raises(MgnError) as ei:
        batched(dict(P, eng=two), T, interval)
    assert ei.value.code == _capi.MGN_E_STATE and "edge set" in str(ei.value)
    two.close()
    cfg = cfg_dict(L=128, mps=2)
    bf = engine_for(cfg, dtype="bf16")
    bf.set_params(make_params(cfg).astype(np.float32))
    bf.set_graph(s, r, N)
    with pytest.raises(MgnError) as ei:
        batched(dict(P, eng=bf), T, interval)
    assert ei.value.code == _capi.MGN_E_STATE and "fp32" in str(ei.value)
    bf.close()
    _, loss = batched(P, T, interval, want_pred=False)
    assert loss == loss_ok
