"""mgn_solver_grad_tsit5 (Engine.solver_grad_tsit5): the loss and discrete-adjoint gradient of one Tsit5 solve on the device (fixed or
adaptive steps, the accepted steps held fixed), against the host composition of mgn_ode_step / mgn_ode_vjp on the same engine
(reference_api.solver_training_tsit5), against the float64 oracle driven by tests/tsit5_adjoint_ref.py over the recorded steps, and
against Engine.rollout("Tsit5", ...).  The fixtures are test_gpu_solver_train.py's.  Run on the MI355X box with `-m gpu`."""
import ctypes as C

import numpy as np
import pytest
import torch   # before the engine's first HIP call (device-array test), or torch finds no GPU afterwards

import tsit5_adjoint_ref as tar
from mgn_amd import MgnError, _capi
from mgn_amd import reference_api as ra
from test_gpu_solver_train import eng_fns, oracle_fns, problem, rel_l2
from util import cfg_dict, engine_for, make_params, rel_max, renumbered

pytestmark = pytest.mark.gpu

# Gradient tolerance against the host composition for adaptive step sequences (the Euler test's is 1e-4, kept for the fixed-step
# cases).  The network's ReLUs make the gradient discontinuous at float32 resolution: the native call forms the stage inputs in float32
# (fused multiply-adds), the host composition in float64 rounded once, and one ulp of difference at a pre-activation next to zero flips a
# ReLU derivative.  Measured on the fixtures here: moving the host composition's VJP inputs by one ulp moved its gradient by 2.3e-4
# relative (hidden_layers = 1), and the native call then agreed with the moved host gradient to 2e-7.  Adaptive runs take more stages
# per window than the fixed-step ones, hence more such points.
ADAPTIVE_TOL = 1e-3


def host(P, stats, save_step=None, **kw):
    rhs, vjp = eng_fns(P)
    return ra.solver_training_tsit5(rhs, vjp, P["gt"][0], P["gt"], stats["step_t"], stats["step_h"], val_mask=P["vm"], save_step=save_step,
                                    **kw)


def test_fixed_step_against_host_oracle_and_central_difference():
    P = problem()
    eng, gt, vm, ns = P["eng"], P["gt"], P["vm"], P["ns"]
    gs, loss, st = eng.solver_grad_tsit5(gt[0], P["onehot"], P["ef_raw"], gt, 0.0, 0.04, 0.01, 5, dt=0.01, adaptive=False, val_mask=vm,
                                         loss_scale=ns)
    assert st["n_accept"] == 4 and st["n_reject"] == 0 and st["n_steps"] == 4 and st["n_rhs"] == 1 + 6 * 4
    assert st["stored_bytes"] == 4 * 6 * P["N"] * 2 * 4
    step_t, step_h, save_step, _ = tar.fixed_steps(0.0, 0.04, 0.01, 0.01, 5)
    assert np.array_equal(st["step_t"], step_t) and np.array_equal(st["step_h"], step_h)
    gs_h, loss_h, _ = host(P, st, n_scale=ns)
    assert abs(loss - loss_h) <= 1e-5 * abs(loss_h), (loss, loss_h)
    assert rel_l2(gs, gs_h) <= 1e-4, rel_l2(gs, gs_h)
    o_rhs, o_vjp, _ = oracle_fns(P)
    gs_o, loss_o, _, _ = tar.tsit5_adjoint(o_rhs, o_vjp, gt[0], gt, step_t, step_h, save_step, 0.01, val_mask=vm, loss_scale=ns)
    assert abs(loss - loss_o) <= 1e-4 * abs(loss_o), (loss, loss_o)
    assert rel_l2(gs, gs_o) <= 5e-3, rel_l2(gs, gs_o)
    d = P["rng"].standard_normal(gs.size)
    d /= np.linalg.norm(d)
    eps = 1e-4

    def loss_at(p):
        r_, _, _ = oracle_fns(P, ps=p)
        return tar.tsit5_adjoint(r_, lambda x, lam: (np.zeros_like(x), np.zeros(gs.size)), gt[0], gt, step_t, step_h, save_step, 0.01,
                                 val_mask=vm, loss_scale=ns)[1]

    p64 = P["ps"].astype(np.float64)
    fd = (loss_at(p64 + eps * d) - loss_at(p64 - eps * d)) / (2 * eps)
    assert abs(fd - float(gs_o @ d)) <= 1e-3 * max(abs(fd), 1e-9), (fd, float(gs_o @ d))
    assert abs(fd - float(gs @ d)) <= 1e-2 * max(abs(fd), 1e-9), (fd, float(gs @ d))


def test_adaptive_no_inflow_matches_rollout_and_the_replayed_steps():
    K = 6
    P = problem(K=K)
    eng, gt, vm, ns = P["eng"], P["gt"], P["vm"], P["ns"]
    t1 = float(np.float32(0.06))
    sol, rs = eng.rollout("Tsit5", gt[0], P["onehot"], P["ef_raw"], 0.0, t1, 0.01, K + 1, val_mask=vm, abstol=1e-6, reltol=1e-3)
    gs, loss, st = eng.solver_grad_tsit5(gt[0], P["onehot"], P["ef_raw"], gt, 0.0, t1, 0.01, K + 1, val_mask=vm, loss_scale=ns,
                                         want_pred=True)
    assert np.array_equal(st["pred"], sol)
    assert (st["n_accept"], st["n_reject"]) == (rs["n_accept"], rs["n_reject"])
    assert st["n_steps"] == st["n_accept"] and len(st["step_h"]) == st["n_accept"] and st["n_accept"] >= K
    save_step = tar.adaptive_saves(st["step_t"], t1, 0.0, 0.01, K + 1)
    gs_h, loss_h, _ = host(P, st, save_step=save_step, n_scale=ns)
    assert abs(loss - loss_h) <= 1e-5 * abs(loss_h), (loss, loss_h)
    assert rel_l2(gs, gs_h) <= ADAPTIVE_TOL, rel_l2(gs, gs_h)
    o_rhs, o_vjp, _ = oracle_fns(P)
    gs_o, loss_o, _, _ = tar.tsit5_adjoint(o_rhs, o_vjp, gt[0], gt, st["step_t"], st["step_h"], save_step, 0.01, val_mask=vm, loss_scale=ns)
    assert abs(loss - loss_o) <= 1e-4 * abs(loss_o), (loss, loss_o)
    assert rel_l2(gs, gs_o) <= 5e-3, rel_l2(gs, gs_o)
    d = P["rng"].standard_normal(gs.size)
    d /= np.linalg.norm(d)
    eps = 1e-4

    def loss_at(p):       # the step sequence frozen
        r_, _, _ = oracle_fns(P, ps=p)
        return tar.tsit5_adjoint(r_, lambda x, lam: (np.zeros_like(x), np.zeros(gs.size)), gt[0], gt, st["step_t"], st["step_h"], save_step,
                                 0.01, val_mask=vm, loss_scale=ns)[1]

    p64 = P["ps"].astype(np.float64)
    fd = (loss_at(p64 + eps * d) - loss_at(p64 - eps * d)) / (2 * eps)
    assert abs(fd - float(gs @ d)) <= 1e-2 * max(abs(fd), 1e-9), (fd, float(gs @ d))


def test_adaptive_inflow_float32_reference_rule():
    K = 6
    P = problem(K=K)
    eng, gt, vm, ns = P["eng"], P["gt"], P["vm"], P["ns"]
    im = (P["node_type"] == 4) | (P["node_type"] == 1)
    assert im.any()
    frames = (gt[0][None] * (1.0 + 0.2 * P["rng"].standard_normal((K + 1, P["N"], 2)))).astype(np.float32)
    kw = dict(val_mask=vm, inflow_mask=im.astype(np.uint8), inflow_data=frames, loss_scale=ns)
    t0, t1 = float(np.float32(0.01)), float(np.float32(0.07))
    # saves (stops) at 0.01 + 0.02 s, frame boundaries at multiples of saves_dt = 0.02: the steps between stops cross them
    gs, loss, st = eng.solver_grad_tsit5(gt[0], P["onehot"], P["ef_raw"], gt[::2][:4], t0, t1, 0.02, 4, dt=0.0, want_pred=True,
                                         inflow_rule="reference", time_type=np.float32, **kw)
    o_rhs, o_vjp, o_rhs_at = oracle_fns(P, inflow_mask=im, frames=frames)
    save_step = tar.adaptive_saves(st["step_t"], t1, t0, 0.02, 4)
    gs_o, loss_o, pred_o, zs = tar.tsit5_adjoint(o_rhs, o_vjp, gt[0], gt[::2][:4], st["step_t"], st["step_h"], save_step, 0.02,
                                                 inflow_rule="reference", time_type=np.float32, rhs_at=o_rhs_at, **kw)
    assert abs(loss - loss_o) <= 1e-4 * abs(loss_o), (loss, loss_o)
    assert rel_l2(gs, gs_o) <= 5e-3, rel_l2(gs, gs_o)
    assert rel_max(st["pred"], pred_o) <= 1e-4
    assert np.array_equal(st["pred"][0], gt[0])         # the state is not overwritten
    # some step's stages read two different frames
    sdt = float(np.float32(0.02))
    crossed = [len({int(np.floor(np.float32(np.float32(t + np.float32(c * h)) / np.float32(sdt)))) for c in ra.TSIT5_C[:6]}) > 1
               for t, h in zip(st["step_t"], st["step_h"])]
    assert any(crossed), (st["step_t"], st["step_h"])


@pytest.mark.parametrize("hidden_layers,ln_dims", [(1, 0), (3, 0), (2, 1)])
def test_hidden_layers_and_ln_all_against_host_composition(hidden_layers, ln_dims):
    P = problem(hidden_layers=hidden_layers, ln_dims=ln_dims)
    eng, gt, vm, ns = P["eng"], P["gt"], P["vm"], P["ns"]
    gs, loss, st = eng.solver_grad_tsit5(gt[0], P["onehot"], P["ef_raw"], gt, 0.0, 0.04, 0.01, 5, val_mask=vm, loss_scale=ns)
    save_step = tar.adaptive_saves(st["step_t"], 0.04, 0.0, 0.01, 5)
    gs_h, loss_h, _ = host(P, st, save_step=save_step, n_scale=ns)
    assert abs(loss - loss_h) <= 1e-5 * abs(loss_h), (loss, loss_h)
    assert rel_l2(gs, gs_h) <= ADAPTIVE_TOL, rel_l2(gs, gs_h)


def test_renumbered_graph_device_tensors_and_repeatable():
    K = 5
    P = problem(K=K, scramble=True, n_points=400)
    eng, gt, vm, ns = P["eng"], P["gt"], P["vm"], P["ns"]
    assert renumbered(eng)
    ct = (gt[-1] + 0.3 * P["rng"].standard_normal(gt[-1].shape)).astype(np.float32)
    kw = dict(val_mask=vm, loss_scale=ns, cont_weight=0.02)
    dev = torch.device("cuda", 0)
    gt_t, ct_t = torch.from_numpy(gt).to(dev), torch.from_numpy(ct).to(dev)
    out_t = torch.full((eng.param_count,), float("nan"), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    _, loss, st = eng.solver_grad_tsit5(gt[0], P["onehot"], P["ef_raw"], gt_t, 0.0, 0.05, 0.01, K + 1, cont_target=ct_t, want_pred=True,
                                        out=out_t, **kw)
    gs = out_t.cpu().numpy()
    gs_n, loss_n, st_n = eng.solver_grad_tsit5(gt[0], P["onehot"], P["ef_raw"], gt, 0.0, 0.05, 0.01, K + 1, cont_target=ct, want_pred=True,
                                               **kw)
    assert loss == loss_n and np.array_equal(gs, gs_n) and np.array_equal(st["pred"], st_n["pred"])
    assert np.array_equal(st["step_h"], st_n["step_h"])
    save_step = tar.adaptive_saves(st["step_t"], 0.05, 0.0, 0.01, K + 1)
    gs_h, loss_h, xs = host(P, st, save_step=save_step, n_scale=ns, cont_target=ct, cont_weight=0.02)
    assert abs(loss - loss_h) <= 1e-5 * abs(loss_h), (loss, loss_h)
    assert rel_l2(gs, gs_h) <= ADAPTIVE_TOL, rel_l2(gs, gs_h)


def test_large_mesh_outside_the_graph_replay_regime():
    K = 2
    P = problem(L=128, mps=2, grid=(130, 100), K=K)        # 13 000 nodes, > 64 k directed edges: one gradient-buffer set, no replay
    eng, gt, vm, ns = P["eng"], P["gt"], P["vm"], P["ns"]
    assert P["s"].size > 2048 * 32
    gs, loss, st = eng.solver_grad_tsit5(gt[0], P["onehot"], P["ef_raw"], gt, 0.0, 0.02, 0.01, K + 1, dt=0.01, adaptive=False, val_mask=vm,
                                         loss_scale=ns)
    gs_h, loss_h, _ = host(P, st, n_scale=ns)
    assert abs(loss - loss_h) <= 1e-5 * abs(loss_h), (loss, loss_h)
    assert rel_l2(gs, gs_h) <= 1e-4, rel_l2(gs, gs_h)


def test_train_step_helpers():
    K = 6
    P = problem(K=K)
    eng, gt, vm = P["eng"], P["gt"], P["vm"]
    gs, loss = ra.train_step_multiple_shooting(eng, gt, P["onehot"], P["ef_raw"], 0.0, 0.01, 0.06, interval_size=3, continuity_term=100,
                                               val_mask=vm, solver="Tsit5", adaptive=False)
    ranges = ra.multiple_shooting_ranges(K + 1, 3)
    gs_d, loss_d = 0.0, 0.0
    for i, (a, b) in enumerate(ranges):
        ct = gt[ranges[i + 1][0]] if i + 1 < len(ranges) else None
        g, l_, _ = eng.solver_grad_tsit5(gt[a], P["onehot"], P["ef_raw"], gt[a:b + 1], float(np.float32(a * 0.01)), float(np.float32(b * 0.01)),
                                         0.01, b - a + 1, dt=0.01, adaptive=False, val_mask=vm, cont_target=ct,
                                         cont_weight=100.0 if ct is not None else 0.0)
        gs_d, loss_d = gs_d + g.astype(np.float64), loss_d + l_
    assert abs(loss - loss_d) <= 1e-6 * abs(loss_d) and np.array_equal(gs, gs_d)
    g1, l1 = ra.train_step_solver_training(eng, gt, P["onehot"], P["ef_raw"], 0.0, 0.01, 0.06, val_mask=vm, n_scale=P["ns"], solver="Tsit5")
    g2, l2, _ = eng.solver_grad_tsit5(gt[0], P["onehot"], P["ef_raw"], gt, 0.0, 0.06, 0.01, K + 1, val_mask=vm, loss_scale=P["ns"])
    assert l1 == l2 and np.array_equal(g1, g2)


def raw_call(eng, d, o, gt, n_grads):
    gs = np.zeros(max(n_grads, 1), np.float32)
    loss = C.c_float()
    return eng.lib.mgn_solver_grad_tsit5(eng.h, C.byref(d), C.byref(o), _capi.f32(gt), None, None, 0.0, _capi.f32(gs), n_grads, C.byref(loss))


def test_refusals_store_limit_and_step_record():
    P = problem(K=4)
    eng, gt = P["eng"], P["gt"]
    args = (gt[0], P["onehot"], P["ef_raw"], gt, 0.0, 0.04, 0.01, 5)
    d = _capi.MgnRolloutDesc()
    d.solver, d.t0, d.t1, d.dt, d.saves_dt, d.n_saves = 0, 0.0, 0.04, 0.01, 0.01, 5
    d.x0, d.node_type_onehot, d.ef_raw = _capi.f32(gt[0]), _capi.f32(P["onehot"]), _capi.f32(P["ef_raw"])
    o = _capi.MgnSolverGradOpts()
    assert raw_call(eng, d, o, gt, eng.param_count) == _capi.MGN_E_ARG           # solver 0
    d.solver = 1
    assert raw_call(eng, d, o, gt, eng.param_count - 1) == _capi.MGN_E_ARG       # n_grads
    with pytest.raises(MgnError) as ei:                  # the sixth save (t = 0.05) is beyond t1
        eng.solver_grad_tsit5(gt[0], P["onehot"], P["ef_raw"], np.concatenate([gt, gt[:1]]), 0.0, 0.04, 0.01, 6)
    assert ei.value.code == _capi.MGN_E_ARG and "reached" in str(ei.value)
    with pytest.raises(MgnError) as ei:
        eng.solver_grad_tsit5(gt[0], P["onehot"], P["ef_raw"], np.concatenate([gt, gt[:1]]), 0.0, 0.04, 0.01, 6, dt=0.01, adaptive=False)
    assert ei.value.code == _capi.MGN_E_ARG and "reached" in str(ei.value)
    stepb = 6 * P["N"] * 2 * 4
    with pytest.raises(MgnError) as ei:
        eng.solver_grad_tsit5(*args, dt=0.01, adaptive=False, max_store_bytes=2 * stepb)
    assert ei.value.code == _capi.MGN_E_OOM and "step 2" in str(ei.value)
    gs, loss, st = eng.solver_grad_tsit5(*args, dt=0.01, adaptive=False, max_store_bytes=4 * stepb)     # the handle still works
    assert st["stored_bytes"] == 4 * stepb
    gs2, loss2, st2 = eng.solver_grad_tsit5(*args, dt=0.01, adaptive=False, step_cap=2)
    assert st2["n_steps"] == 4 and len(st2["step_h"]) == 2 and np.array_equal(st2["step_t"], st["step_t"][:2])
    assert loss2 == loss and np.array_equal(gs2, gs)
    with pytest.raises(MgnError) as ei:
        eng.solver_grad(*args[:6], 0.01, 0.01, 5, solver="Tsit5")
    assert ei.value.code == _capi.MGN_E_UNSUPPORTED
    s, r, N = P["s"], P["r"], P["N"]
    cfg = cfg_dict(L=128, mps=2)
    bf = engine_for(cfg, dtype="bf16")
    bf.set_params(make_params(cfg).astype(np.float32))
    bf.set_graph(s, r, N)
    with pytest.raises(MgnError) as ei:
        bf.solver_grad_tsit5(*args)
    assert ei.value.code == _capi.MGN_E_STATE and "fp32" in str(ei.value)
    bf.close()
    two = engine_for(P["cfg"], Fe2=3)
    two.set_params(np.zeros(two.param_count, np.float32))
    two.set_graph(s, r, N)
    two.set_edge_set(1, r[:10], s[:10])
    two.set_edge_features(1, np.zeros((10, 3), np.float32))
    with pytest.raises(MgnError) as ei:
        two.solver_grad_tsit5(*args)
    assert ei.value.code == _capi.MGN_E_STATE and "edge set" in str(ei.value)
    two.close()
    part = engine_for(P["cfg"], rank=0, nranks=2)
    part.set_params(P["ps"])
    part.set_graph(s, r, N)
    with pytest.raises(MgnError) as ei:
        part.solver_grad_tsit5(*args)
    assert ei.value.code == _capi.MGN_E_STATE and "partition" in str(ei.value)
    part.close()
