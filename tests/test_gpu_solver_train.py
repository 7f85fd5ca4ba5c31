"""mgn_solver_grad (Engine.solver_grad): the loss and discrete-adjoint gradient of one fixed-step Euler solve on the device, against the
host composition of mgn_ode_step / mgn_ode_vjp on the same engine and against the float64 oracle driven by tests/solver_adjoint_ref.py.
Run on the MI355X box with `-m gpu`."""
import ctypes as C

import numpy as np
import pytest
import torch   # before the engine's first HIP call (device-array test), or torch finds no GPU afterwards

import mgn_oracle as orc
import solver_adjoint_ref as sar
from mgn_amd import MgnError, _capi, synth
from mgn_amd import reference_api as ra
from util import cfg_dict, engine_for, make_params, rel_max, renumbered, scatter_labels

pytestmark = pytest.mark.gpu


def rel_l2(a, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.linalg.norm(np.asarray(a, np.float64) - ref) / max(np.linalg.norm(ref), 1e-30))


def problem(L=64, mps=2, hidden_layers=2, ln_dims=0, n_points=150, K=4, scramble=False, grid=None, seed=6):
    cfg = cfg_dict(L=L, mps=mps)
    cfg["hidden_layers"] = hidden_layers
    if grid is None:
        pos, cells, node_type, vel = synth.mesh_cyl(1234, n_points)
    else:
        pos, cells = synth.grid_mesh(*grid, 1234)
        rng0 = np.random.default_rng(1)
        node_type = rng0.choice([0, 1, 4, 5, 6], pos.shape[0], p=[0.8, 0.05, 0.05, 0.05, 0.05]).astype(np.int32)
        vel = rng0.standard_normal((pos.shape[0], 2)).astype(np.float32)
    s, r = synth.cells_to_edges(cells)
    if scramble:
        pos, s, r, perm = scatter_labels(pos, s, r, seed=3)
        inv = np.argsort(perm)
        node_type, vel = node_type[inv], vel[inv]
    N = pos.shape[0]
    rng = np.random.default_rng(seed)
    onehot = orc.one_hot(node_type, 7, 0).astype(np.float32)
    ef_raw = orc.edge_features(pos, s, r).astype(np.float32)
    gt = (vel[None] * (1.0 + 0.05 * rng.standard_normal((K + 1, N, 2)))).astype(np.float32)
    P = dict(cfg=cfg, s=s, r=r, N=N, onehot=onehot, ef_raw=ef_raw, gt=gt, node_type=node_type, rng=rng,
             n_norm=orc.NormMeanStd(np.array([1.0, 0.1]), np.array([0.4, 0.2])), t_norm=orc.NormMinMax(0.0, 1.0),
             e_norm=orc.NormMeanStd(ef_raw.mean(0), ef_raw.std(0)), o_norm=orc.NormMeanStd(np.array([0.01, -0.02]), np.array([5.0, 4.0])),
             vm=np.isin(node_type, [0, 5]).astype(np.float32))
    P["ps"] = make_params(cfg).astype(np.float32)
    ns, nsh = P["n_norm"].affine(2)
    ts, tsh = P["t_norm"].affine(7)
    es, esh = P["e_norm"].affine(3)
    P["ns"] = ns
    eng = engine_for(cfg, ln_dims=ln_dims)
    eng.set_params(P["ps"])
    eng.set_graph(s, r, N)
    eng.set_norms(node=(np.concatenate([ns, ts]), np.concatenate([nsh, tsh])), edge=(es, esh), out=(P["o_norm"].std, P["o_norm"].mean))
    P["eng"] = eng
    return P


def eng_fns(P):
    eng, oh, ef, vm = P["eng"], P["onehot"], P["ef_raw"], P["vm"]
    return (lambda x: eng.ode_step(x, oh, ef, vm)), (lambda x, lam: eng.ode_vjp(x, oh, ef, lam, val_mask=vm)[:2])


def oracle_fns(P, ps=None, inflow_mask=None, frames=None):
    ps = P["ps"] if ps is None else ps
    args = (P["onehot"], P["ef_raw"], P["s"], P["r"], P["n_norm"], P["t_norm"], P["e_norm"], P["o_norm"])
    vm2 = P["vm"][:, None].astype(np.float64)

    def rhs(x):
        return orc.ode_rhs(ps, P["cfg"], x, *args, vm2)

    def rhs_at(x, fr):
        if fr is None:
            return rhs(x)
        return orc.ode_rhs(ps, P["cfg"], x, *args, vm2, inflow_mask=inflow_mask, inflow_values=frames[fr])

    def vjp(x, lam):
        return orc.ode_vjp(ps, P["cfg"], x, *args, P["vm"], lam)[:2]

    return rhs, vjp, rhs_at


def test_native_matches_host_composition_and_oracle():
    P = problem()
    eng, gt, vm, ns = P["eng"], P["gt"], P["vm"], P["ns"]
    gs, loss = eng.solver_grad(gt[0], P["onehot"], P["ef_raw"], gt, 0.0, 0.04, 0.01, 0.01, 5, val_mask=vm, loss_scale=ns)
    rhs, vjp = eng_fns(P)
    gs_h, loss_h, _ = ra.solver_training_euler(rhs, vjp, gt[0], gt, 0.01, vm, ns)
    assert abs(loss - loss_h) <= 1e-5 * abs(loss_h), (loss, loss_h)
    assert rel_l2(gs, gs_h) <= 1e-4, rel_l2(gs, gs_h)
    o_rhs, o_vjp, _ = oracle_fns(P)
    gs_o, loss_o, _, _ = sar.euler_adjoint(o_rhs, o_vjp, gt[0], gt, 0.0, 0.04, 0.01, 0.01, 5, val_mask=vm, loss_scale=ns)
    assert abs(loss - loss_o) <= 1e-4 * abs(loss_o), (loss, loss_o)
    assert rel_l2(gs, gs_o) <= 5e-3, rel_l2(gs, gs_o)
    # the oracle's adjoint is the gradient of its loss: directional central difference
    d = P["rng"].standard_normal(gs.size)
    d /= np.linalg.norm(d)
    eps = 1e-4

    def loss_at(p):
        r_, _, _ = oracle_fns(P, ps=p)
        return sar.euler_adjoint(r_, lambda x, lam: (np.zeros_like(x), np.zeros(gs.size)), gt[0], gt, 0.0, 0.04, 0.01, 0.01, 5,
                                 val_mask=vm, loss_scale=ns)[1]

    p64 = P["ps"].astype(np.float64)
    fd = (loss_at(p64 + eps * d) - loss_at(p64 - eps * d)) / (2 * eps)
    assert abs(fd - float(gs_o @ d)) <= 1e-3 * max(abs(fd), 1e-9), (fd, float(gs_o @ d))
    assert abs(fd - float(gs @ d)) <= 1e-2 * max(abs(fd), 1e-9), (fd, float(gs @ d))


def test_inflow_copy_frames_float32_reference_rule():
    K = 6
    P = problem(K=K)
    eng, gt, vm, ns = P["eng"], P["gt"], P["vm"], P["ns"]
    im = (P["node_type"] == 4) | (P["node_type"] == 1)
    assert im.any()
    frames = (gt[0][None] * (1.0 + 0.2 * P["rng"].standard_normal((K + 1, P["N"], 2)))).astype(np.float32)
    kw = dict(val_mask=vm, inflow_mask=im.astype(np.uint8), inflow_data=frames, loss_scale=ns)
    gs, loss, pred = eng.solver_grad(gt[0], P["onehot"], P["ef_raw"], gt, 0.0, 0.06, 0.01, 0.01, K + 1, want_pred=True,
                                     inflow_rule="reference", time_type=np.float32, **kw)
    o_rhs, o_vjp, o_rhs_at = oracle_fns(P, inflow_mask=im, frames=frames)
    gs_o, loss_o, pred_o, xin = sar.euler_adjoint(o_rhs, o_vjp, gt[0], gt, 0.0, 0.06, 0.01, 0.01, K + 1, inflow_rule="reference",
                                                  time_type=np.float32, rhs_at=o_rhs_at, **kw)
    assert abs(loss - loss_o) <= 1e-4 * abs(loss_o), (loss, loss_o)
    assert rel_l2(gs, gs_o) <= 5e-3, rel_l2(gs, gs_o)
    assert rel_max(pred, pred_o) <= 1e-4
    # the states are not overwritten (the rows the RHS saw were): the saved inflow rows are x0's plus the integrated change
    assert np.array_equal(pred[0], gt[0])
    assert not np.allclose(pred[1][im], frames[0][im], rtol=1e-3, atol=1e-4)
    assert np.array_equal(xin[0][im], frames[0][im].astype(np.float64))


def test_substeps_no_loss_scale_continuity_term():
    P = problem()
    eng, gt, vm = P["eng"], P["gt"], P["vm"]
    ct = (gt[-1] + 0.3 * P["rng"].standard_normal(gt[-1].shape)).astype(np.float32)
    kw = dict(val_mask=vm, cont_target=ct, cont_weight=0.05)
    gs, loss = eng.solver_grad(gt[0], P["onehot"], P["ef_raw"], gt, 0.0, 0.04, 0.005, 0.01, 5, **kw)
    o_rhs, o_vjp, _ = oracle_fns(P)
    gs_o, loss_o, _, _ = sar.euler_adjoint(o_rhs, o_vjp, gt[0], gt, 0.0, 0.04, 0.005, 0.01, 5, **kw)
    assert abs(loss - loss_o) <= 1e-4 * abs(loss_o), (loss, loss_o)
    assert rel_l2(gs, gs_o) <= 5e-3, rel_l2(gs, gs_o)
    gs0, loss0 = eng.solver_grad(gt[0], P["onehot"], P["ef_raw"], gt, 0.0, 0.04, 0.005, 0.01, 5, val_mask=vm)
    assert loss > loss0 and not np.array_equal(gs, gs0)      # the continuity term is in


def test_multiple_shooting_matches_driver_over_windows():
    K = 6
    P = problem(K=K)
    eng, gt, vm = P["eng"], P["gt"], P["vm"]
    gs, loss = ra.train_step_multiple_shooting(eng, gt, P["onehot"], P["ef_raw"], 0.0, 0.01, 0.06, interval_size=3, continuity_term=100,
                                               val_mask=vm)
    rhs, vjp = eng_fns(P)
    ranges = ra.multiple_shooting_ranges(K + 1, 3)
    assert ranges == [(0, 2), (2, 4), (4, 6)]
    gs_d, loss_d = 0.0, 0.0
    for i, (a, b) in enumerate(ranges):
        ct = gt[ranges[i + 1][0]] if i + 1 < len(ranges) else None
        g, l_, _, _ = sar.euler_adjoint(rhs, vjp, gt[a], gt[a:b + 1], float(np.float32(a * 0.01)), float(np.float32(b * 0.01)), 0.01, 0.01,
                                        b - a + 1, val_mask=vm, cont_target=ct, cont_weight=100.0 if ct is not None else 0.0)
        gs_d, loss_d = gs_d + g, loss_d + l_
    assert abs(loss - loss_d) <= 1e-5 * abs(loss_d), (loss, loss_d)
    assert rel_l2(gs, gs_d) <= 1e-4, rel_l2(gs, gs_d)
    # SolverTraining's helper is one window over the whole trajectory with the normaliser's scale
    g1, l1 = ra.train_step_solver_training(eng, gt, P["onehot"], P["ef_raw"], 0.0, 0.01, 0.06, val_mask=vm, n_scale=P["ns"])
    g2, l2 = eng.solver_grad(gt[0], P["onehot"], P["ef_raw"], gt, 0.0, 0.06, 0.01, 0.01, K + 1, val_mask=vm, loss_scale=P["ns"])
    assert l1 == l2 and np.array_equal(g1, g2)


def test_pred_bit_identical_to_rollout_and_repeatable():
    K = 10
    P = problem(K=K)
    eng, gt, vm = P["eng"], P["gt"], P["vm"]
    sol, _ = eng.rollout("Euler", gt[0], P["onehot"], P["ef_raw"], 0.0, 0.1, 0.01, K + 1, dt=0.01, val_mask=vm)
    g1, l1, pred = eng.solver_grad(gt[0], P["onehot"], P["ef_raw"], gt, 0.0, 0.1, 0.01, 0.01, K + 1, val_mask=vm, loss_scale=P["ns"],
                                   want_pred=True)
    assert np.array_equal(pred, sol)
    g2, l2 = eng.solver_grad(gt[0], P["onehot"], P["ef_raw"], gt, 0.0, 0.1, 0.01, 0.01, K + 1, val_mask=vm, loss_scale=P["ns"])
    assert l1 == l2 and np.array_equal(g1, g2)
    sol2, _ = eng.rollout("Euler", gt[0], P["onehot"], P["ef_raw"], 0.0, 0.1, 0.01, K + 1, dt=0.01, val_mask=vm)
    assert np.array_equal(sol, sol2)        # the rollout is not disturbed by the training calls in between


@pytest.mark.parametrize("hidden_layers,ln_dims", [(3, 0), (2, 1), (1, 1)])
def test_hidden_layers_and_ln_all_against_host_composition(hidden_layers, ln_dims):
    P = problem(hidden_layers=hidden_layers, ln_dims=ln_dims)
    eng, gt, vm, ns = P["eng"], P["gt"], P["vm"], P["ns"]
    gs, loss = eng.solver_grad(gt[0], P["onehot"], P["ef_raw"], gt, 0.0, 0.04, 0.01, 0.01, 5, val_mask=vm, loss_scale=ns)
    rhs, vjp = eng_fns(P)
    gs_h, loss_h, _ = ra.solver_training_euler(rhs, vjp, gt[0], gt, 0.01, vm, ns)
    assert abs(loss - loss_h) <= 1e-5 * abs(loss_h), (loss, loss_h)
    assert rel_l2(gs, gs_h) <= 1e-4, rel_l2(gs, gs_h)


def test_renumbered_graph_and_device_tensors():
    K = 5
    P = problem(K=K, scramble=True, n_points=400)
    eng, gt, vm, ns = P["eng"], P["gt"], P["vm"], P["ns"]
    assert renumbered(eng)
    im = (P["node_type"] == 4) | (P["node_type"] == 1)
    frames = (gt[0][None] * (1.0 + 0.2 * P["rng"].standard_normal((K + 1, P["N"], 2)))).astype(np.float32)
    ct = (gt[-1] + 0.3 * P["rng"].standard_normal(gt[-1].shape)).astype(np.float32)
    kw = dict(val_mask=vm, inflow_mask=im.astype(np.uint8), inflow_data=frames, loss_scale=ns, cont_weight=0.02)
    dev = torch.device("cuda", 0)
    gt_t = torch.from_numpy(gt).to(dev)
    ct_t = torch.from_numpy(ct).to(dev)
    out_t = torch.full((eng.param_count,), float("nan"), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    _, loss, pred = eng.solver_grad(gt[0], P["onehot"], P["ef_raw"], gt_t, 0.0, 0.05, 0.01, 0.01, K + 1, cont_target=ct_t, want_pred=True,
                                    out=out_t, **kw)
    gs = out_t.cpu().numpy()
    gs_n, loss_n, pred_n = eng.solver_grad(gt[0], P["onehot"], P["ef_raw"], gt, 0.0, 0.05, 0.01, 0.01, K + 1, cont_target=ct, want_pred=True,
                                           **kw)
    assert loss == loss_n and np.array_equal(gs, gs_n) and np.array_equal(pred, pred_n)   # host and device arrays: the same call
    rhs, vjp = eng_fns(P)
    gs_h, loss_h, pred_h, _ = sar.euler_adjoint(rhs, vjp, gt[0], gt, 0.0, 0.05, 0.01, 0.01, K + 1, cont_target=ct, **kw)
    assert abs(loss - loss_h) <= 1e-5 * abs(loss_h), (loss, loss_h)
    assert rel_l2(gs, gs_h) <= 1e-4, rel_l2(gs, gs_h)
    assert rel_max(pred, pred_h) <= 1e-5


def test_large_mesh_outside_the_graph_replay_regime():
    K = 3
    P = problem(L=128, mps=2, grid=(130, 100), K=K)        # 13 000 nodes, > 64 k directed edges: one gradient-buffer set, no replay
    eng, gt, vm, ns = P["eng"], P["gt"], P["vm"], P["ns"]
    assert P["s"].size > 2048 * 32
    gs, loss = eng.solver_grad(gt[0], P["onehot"], P["ef_raw"], gt, 0.0, 0.03, 0.01, 0.01, K + 1, val_mask=vm, loss_scale=ns)
    rhs, vjp = eng_fns(P)
    gs_h, loss_h, _ = ra.solver_training_euler(rhs, vjp, gt[0], gt, 0.01, vm, ns)
    assert abs(loss - loss_h) <= 1e-5 * abs(loss_h), (loss, loss_h)
    assert rel_l2(gs, gs_h) <= 1e-4, rel_l2(gs, gs_h)


def raw_call(eng, x0, oh, ef, gt, n_grads):
    """mgn_solver_grad through ctypes with the arguments as given (NULL gt, a wrong n_grads)."""
    d = _capi.MgnRolloutDesc()
    d.solver, d.t0, d.t1, d.dt, d.saves_dt, d.n_saves = 0, 0.0, 0.02, 0.01, 0.01, 3
    d.x0, d.node_type_onehot, d.ef_raw = _capi.f32(x0), _capi.f32(oh), _capi.f32(ef)
    gs = np.zeros(max(n_grads, 1), np.float32)
    loss = C.c_float()
    return eng.lib.mgn_solver_grad(eng.h, C.byref(d), _capi.f32(gt), None, None, 0.0, _capi.f32(gs), n_grads, C.byref(loss))


def test_refusals():
    P = problem(K=2)
    eng, gt = P["eng"], P["gt"]
    args = (gt[0], P["onehot"], P["ef_raw"], gt, 0.0, 0.02, 0.01, 0.01, 3)
    with pytest.raises(MgnError) as ei:
        eng.solver_grad(*args, solver="Tsit5")
    assert ei.value.code == _capi.MGN_E_UNSUPPORTED
    with pytest.raises(MgnError) as ei:                  # the fourth save (t = 0.03) is beyond t1
        eng.solver_grad(gt[0], P["onehot"], P["ef_raw"], np.concatenate([gt, gt[:1]]), 0.0, 0.02, 0.01, 0.01, 4)
    assert ei.value.code == _capi.MGN_E_ARG and "reached" in str(ei.value)
    assert raw_call(eng, gt[0], P["onehot"], P["ef_raw"], gt, eng.param_count - 1) == _capi.MGN_E_ARG
    assert raw_call(eng, gt[0], P["onehot"], P["ef_raw"], None, eng.param_count) == _capi.MGN_E_ARG
    eng.solver_grad(*args)                               # and the handle still works
    s, r, N = P["s"], P["r"], P["N"]
    cfg = cfg_dict(L=128, mps=2)
    bf = engine_for(cfg, dtype="bf16")
    bf.set_params(make_params(cfg).astype(np.float32))
    bf.set_graph(s, r, N)
    with pytest.raises(MgnError) as ei:
        bf.solver_grad(*args)
    assert ei.value.code == _capi.MGN_E_STATE and "fp32" in str(ei.value)
    bf.close()
    two = engine_for(P["cfg"], Fe2=3)
    two.set_params(np.zeros(two.param_count, np.float32))
    two.set_graph(s, r, N)
    two.set_edge_set(1, r[:10], s[:10])
    two.set_edge_features(1, np.zeros((10, 3), np.float32))
    with pytest.raises(MgnError) as ei:
        two.solver_grad(*args)
    assert ei.value.code == _capi.MGN_E_STATE and "edge set" in str(ei.value)
    two.close()
    part = engine_for(P["cfg"], rank=0, nranks=2)
    part.set_params(P["ps"])
    part.set_graph(s, r, N)
    with pytest.raises(MgnError) as ei:
        part.solver_grad(*args)
    assert ei.value.code == _capi.MGN_E_STATE and "partition" in str(ei.value)
    part.close()
