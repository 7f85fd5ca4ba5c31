"""mgn_solver_grad_tsit5 with MGN_TSIT5_DENSE_SAVES (Engine.solver_grad_tsit5(dense_saves=True)): a Tsit5 window solved with saveat and no
tstops -- the only stop is t1, the saves between steps come from Tsit5's dense output -- and its discrete adjoint with the steps and the
interpolation points held fixed.  Against the host composition of mgn_ode_step / mgn_ode_vjp on the same engine (tests/tsit5_dense_ref.py
driven by the engine's own right-hand side and VJP, float32 in and out), against the float64 oracle through the same driver over the
recorded steps, against a directional central difference of the oracle's loss with steps and theta frozen, and against the tstops modes
where the two must agree.  The fixtures and tolerances are test_gpu_solver_train_tsit5.py's.  Run on the MI355X box with `-m gpu`.

Every window ends on the save grid's own last point, t_at(n_saves - 1) = float32(i * float32(0.01)), which for i = 5 lies an ulp below
float32(0.05): a t1 an ulp beyond the last save time makes that save an interpolated one at theta = 1 - 4e-7 instead of the final state.

Measured on the MI355X (every test prints its figures before it asserts), relative errors, gradient in rel-L2:
  fixed dt = 0.025, 6 saves:      host composition loss 1.1e-7 gradient 4.0e-5; oracle loss 2.0e-7 gradient 6.5e-7 pred 4.2e-7;
                                  central difference 3.057932e-3 against the native 3.074441e-3 (5.4e-3; the oracle's own adjoint 3.074435e-3)
  fixed dt = 0.015, inflow:       oracle loss 1.7e-7 gradient 7.8e-7 pred 3.5e-7
  adaptive, 7 saves, reltol 1e-3: 5 accepted steps (0 rejected, 32 right-hand sides) against 6 (0 rejected, 38) with tstops = saves; saves
                                  1 .. 5 interpolated (two inside the first step of 0.0239); host composition loss 6.5e-8 gradient 4.8e-5;
                                  oracle loss 1.6e-7 gradient 5.3e-7 pred 4.2e-7; central difference 4.665483e-3 against the native 4.663765e-3
  hidden_layers 1 / 3 (seed 9) / ln_dims 1: host composition gradient 5.2e-7 / 8.6e-7 / 1.0e-6;  renumbered, device tensors: 1.0e-5
The seed of the hidden_layers = 3 case: see the note above its test."""
import ctypes as C

import numpy as np
import pytest
import torch   # before the engine's first HIP call (device-array test), or torch finds no GPU afterwards

import tsit5_dense_ref as tdr
from mgn_amd import MgnError, _capi
from mgn_amd import reference_api as ra
from test_gpu_solver_train import oracle_fns, problem, rel_l2
from test_gpu_solver_train_tsit5 import ADAPTIVE_TOL
from util import rel_max, renumbered

pytestmark = pytest.mark.gpu

F32 = np.float32
SDT = 0.01
# the adaptive fixture's relative tolerance: rollout's default.  (Raised only if no free step straddles a save on the device.)
ADAPTIVE_RELTOL = 1e-3


def t_at(i, t0=0.0, sdt=SDT):
    """save time i in the float32 time type, as the library forms it"""
    return float(F32(float(F32(t0)) + i * float(F32(sdt))))


def host_fns(P):
    eng, oh, ef, vm = P["eng"], P["onehot"], P["ef_raw"], P["vm"]
    return (lambda x: eng.ode_step(np.asarray(x, F32), oh, ef, vm)), \
           (lambda x, lam: eng.ode_vjp(np.asarray(x, F32), oh, ef, np.asarray(lam, F32), val_mask=vm)[:2])


def plan_of(st, t0, t1, n_saves, sdt=SDT, time_type=F32):
    return tdr.dense_plan(st["step_t"], st["step_h"], t1, t0, sdt, n_saves, time_type)


def check(P, gt, st, gs, loss, plan, t1, tol_host, what, inflow=None, fd=True, host=True, **kw):
    """the comparisons of one dense call: host composition, float64 oracle, directional central difference (steps and theta frozen)"""
    vm, ns = P["vm"], P["ns"]
    common = dict(val_mask=vm, loss_scale=ns, **kw)
    if host:
        rhs, vjp = host_fns(P)
        gs_h, loss_h, _, _, _ = tdr.tsit5_dense_adjoint(rhs, vjp, gt[0], gt, st["step_t"], st["step_h"], t1, plan, SDT, **common)
        print("%s: host composition: loss %.2e gradient %.2e" % (what, abs(loss - loss_h) / abs(loss_h), rel_l2(gs, gs_h)))
        assert abs(loss - loss_h) <= 1e-5 * abs(loss_h), (loss, loss_h)
        assert rel_l2(gs, gs_h) <= tol_host, rel_l2(gs, gs_h)
    okw = dict(inflow_mask=inflow[0], frames=inflow[1]) if inflow else {}
    ikw = dict(inflow_mask=inflow[0], inflow_data=inflow[1], inflow_rule="reference") if inflow else {}
    o_rhs, o_vjp, o_rhs_at = oracle_fns(P, **okw)
    gs_o, loss_o, pred_o, _, _ = tdr.tsit5_dense_adjoint(o_rhs, o_vjp, gt[0], gt, st["step_t"], st["step_h"], t1, plan, SDT,
                                                         rhs_at=o_rhs_at if inflow else None, **common, **ikw)
    print("%s: oracle: loss %.2e gradient %.2e pred %.2e" % (what, abs(loss - loss_o) / abs(loss_o), rel_l2(gs, gs_o),
                                                          rel_max(st["pred"], pred_o)))
    assert abs(loss - loss_o) <= 1e-4 * abs(loss_o), (loss, loss_o)
    assert rel_l2(gs, gs_o) <= 5e-3, rel_l2(gs, gs_o)
    assert rel_max(st["pred"], pred_o) <= 1e-4
    if not fd:
        return
    d = np.random.default_rng(11).standard_normal(gs.size)
    d /= np.linalg.norm(d)
    eps = 1e-4
    no_vjp = lambda x, lam: (np.zeros_like(x), np.zeros(gs.size))      # noqa: E731  (the loss alone)

    def loss_at(p):
        r_, _, ra_ = oracle_fns(P, ps=p, **okw)
        return tdr.tsit5_dense_adjoint(r_, no_vjp, gt[0], gt, st["step_t"], st["step_h"], t1, plan, SDT, rhs_at=ra_ if inflow else None,
                                       **common, **ikw)[1]

    p64 = P["ps"].astype(np.float64)
    fdv = (loss_at(p64 + eps * d) - loss_at(p64 - eps * d)) / (2 * eps)
    print("%s: central difference %.6e, oracle adjoint %.6e, native %.6e" % (what, fdv, float(gs_o @ d), float(gs @ d)))
    assert abs(fdv - float(gs @ d)) <= 1e-2 * max(abs(fdv), 1e-9), (fdv, float(gs @ d))


def test_fixed_steps_across_the_saves():
    """dt = 0.025 over six saves of 0.01: two steps; saves 1, 2 inside the first (theta 0.4, 0.8), 3, 4 inside the last (0.2, 0.6: the extra
    VJP at z_{K,1}; the first step's b_7 term into stage 1 of the second), save 5 is x_K"""
    P = problem(K=5)
    eng, gt, vm, ns = P["eng"], P["gt"], P["vm"], P["ns"]
    t1 = t_at(5)
    gs, loss, st = eng.solver_grad_tsit5(gt[0], P["onehot"], P["ef_raw"], gt, 0.0, t1, SDT, 6, dt=0.025, adaptive=False, dense_saves=True,
                                         val_mask=vm, loss_scale=ns, want_pred=True)
    h = float(F32(0.025))
    assert st["step_h"].tolist() == [h, h] and st["step_t"].tolist() == [0.0, h]
    assert st["n_accept"] == 2 and st["n_reject"] == 0 and st["n_steps"] == 2 and st["n_rhs"] == 1 + 6 * 2
    assert st["stored_bytes"] == (2 * 6 + 7) * P["N"] * 2 * 4
    plan = plan_of(st, 0.0, t1, 6)
    assert [(i, hit) for i, _, hit in plan] == [(0, True), (0, False), (0, False), (1, False), (1, False), (2, True)]
    assert np.allclose([th for _, th, hit in plan if not hit], [0.4, 0.8, 0.2, 0.6], atol=1e-6)
    assert np.array_equal(st["pred"][0], gt[0])
    check(P, gt, st, gs, loss, plan, t1, 1e-4, "fixed 0.025")
    # the same bits on a second call
    gs2, loss2, st2 = eng.solver_grad_tsit5(gt[0], P["onehot"], P["ef_raw"], gt, 0.0, t1, SDT, 6, dt=0.025, adaptive=False, dense_saves=True,
                                            val_mask=vm, loss_scale=ns, want_pred=True)
    assert loss2 == loss and np.array_equal(gs2, gs) and np.array_equal(st2["pred"], st["pred"])


# A single step of 0.07 moves the stage inputs far, and the ground-truth seeds 6, 7, 8 and 10 each leave a ReLU pre-activation next to
# zero (the one-ulp experiment, as for the hidden_layers = 3 case below).  Measured on the MI355X, gradient rel-L2: the host composition's
# own gradient when x0 moves by one ulp up / down: seed 6: 5.3e-6 / 5.9e-4, 7: 3.8e-3 / 4.4e-3, 8: 2.1e-6 / 2.4e-3, 9: 4.4e-6 / 6.0e-6,
# 10: 3.6e-3 / 3.4e-3.  Seed 6: native against host 5.9e-4, against the host moved one ulp down 5.3e-6.  Seed 9, the one stable in both
# directions: native against host 3.9e-6, against the float64 oracle 4.8e-6.
def test_more_saves_inside_one_step_than_one_launch_takes():
    """dt = 0.08 past t1 = 0.07: one step, cut to 0.07, with saves 1 .. 6 inside it -- the adjoint kernel takes four saves per launch, so
    the second launch adds to the first's sums -- and the extra VJP at z_{K,1} is the sweep's first"""
    K = 7
    P = problem(K=K, seed=9)
    eng, gt, vm, ns = P["eng"], P["gt"], P["vm"], P["ns"]
    t1 = t_at(K)
    gs, loss, st = eng.solver_grad_tsit5(gt[0], P["onehot"], P["ef_raw"], gt, 0.0, t1, SDT, K + 1, dt=0.08, adaptive=False, dense_saves=True,
                                         val_mask=vm, loss_scale=ns, want_pred=True)
    assert st["n_steps"] == 1 and st["step_h"].tolist() == [t1] and st["n_rhs"] == 7
    plan = plan_of(st, 0.0, t1, K + 1)
    assert [(i, hit) for i, _, hit in plan] == [(0, True)] + [(0, False)] * 6 + [(1, True)]
    check(P, gt, st, gs, loss, plan, t1, 1e-4, "one step, six saves inside", fd=False)


def test_fixed_steps_cut_at_t1_with_inflow_frames():
    """dt = 0.015 to t1 = 0.04: the last step is cut to 0.01; the inflow rows come from frames of 0.01 s, so the stages of a step read
    different frames; float32 times, the reference's frame rule"""
    P = problem(K=5)
    eng, gt, vm, ns = P["eng"], P["gt"], P["vm"], P["ns"]
    im = (P["node_type"] == 4) | (P["node_type"] == 1)
    assert im.any()
    frames = (gt[0][None] * (1.0 + 0.2 * P["rng"].standard_normal((6, P["N"], 2)))).astype(F32)
    t1 = t_at(4)
    gs, loss, st = eng.solver_grad_tsit5(gt[0], P["onehot"], P["ef_raw"], gt[:5], 0.0, t1, SDT, 5, dt=0.015, adaptive=False, dense_saves=True,
                                         val_mask=vm, loss_scale=ns, inflow_mask=im.astype(np.uint8), inflow_data=frames,
                                         inflow_rule="reference", time_type=F32, want_pred=True)
    st_r, sh_r, te_r = tdr.fixed_dense_steps(0.0, t1, 0.015, SDT, F32)
    assert st["step_t"].tolist() == st_r and st["step_h"].tolist() == sh_r and te_r == t1
    assert st["n_steps"] == 3 and abs(st["step_h"][2] - 0.01) < 1e-7 and st["step_h"][0] == float(F32(0.015))
    plan = plan_of(st, 0.0, t1, 5)
    assert [(i, hit) for i, _, hit in plan] == [(0, True), (0, False), (1, False), (2, True), (3, True)]
    assert np.array_equal(st["pred"][0], gt[0])          # the state is not overwritten
    sdt = float(F32(SDT))
    crossed = [len({int(np.floor(F32(F32(t + F32(c * h)) / F32(sdt)))) for c in ra.TSIT5_C[:6]}) > 1
               for t, h in zip(st["step_t"], st["step_h"])]
    assert any(crossed), (st["step_t"], st["step_h"])
    check(P, gt[:5], st, gs, loss, plan, t1, None, "fixed 0.015 inflow", inflow=(im, frames), fd=False, host=False)


def test_adaptive_free_steps():
    """solve(prob, Tsit5(); saveat = saves): the controller steps freely to t1.  Fewer accepted steps than with tstops = saves on the same
    inputs, at least one save interpolated, the last save the final state"""
    K = 6
    P = problem(K=K)
    eng, gt, vm, ns = P["eng"], P["gt"], P["vm"], P["ns"]
    t1 = t_at(K)
    args = (gt[0], P["onehot"], P["ef_raw"], gt, 0.0, t1, SDT, K + 1)
    kw = dict(val_mask=vm, loss_scale=ns, abstol=1e-6, reltol=ADAPTIVE_RELTOL, want_pred=True)
    _, _, st_stops = eng.solver_grad_tsit5(*args, **kw)
    gs, loss, st = eng.solver_grad_tsit5(*args, dense_saves=True, **kw)
    print("accepted steps: tstops = saves %d (%d rejected), free %d (%d rejected); right-hand sides %d / %d"
          % (st_stops["n_accept"], st_stops["n_reject"], st["n_accept"], st["n_reject"], st_stops["n_rhs"], st["n_rhs"]))
    print("free steps:", st["step_h"].tolist())
    assert st["n_accept"] < st_stops["n_accept"], (st["n_accept"], st_stops["n_accept"])
    assert st["n_steps"] == st["n_accept"] == len(st["step_h"])
    plan = plan_of(st, 0.0, t1, K + 1)
    print("plan:", plan)
    assert any(not hit for _, _, hit in plan)                        # a condition of the fixture: a free step straddles a save
    assert plan[-1] == (st["n_steps"], None, True)                   # the last save is the final state
    assert abs(st["step_t"][-1] + st["step_h"][-1] - t1) <= 1e-7
    assert np.array_equal(st["pred"][0], gt[0])
    check(P, gt, st, gs, loss, plan, t1, ADAPTIVE_TOL, "adaptive")
    gs2, loss2, st2 = eng.solver_grad_tsit5(*args, dense_saves=True, **kw)
    assert loss2 == loss and np.array_equal(gs2, gs) and np.array_equal(st2["pred"], st["pred"])
    assert np.array_equal(st2["step_h"], st["step_h"])


def test_dense_and_tstops_agree_when_every_save_is_a_step_end():
    P = problem()
    eng, gt, vm, ns = P["eng"], P["gt"], P["vm"], P["ns"]
    ct = (gt[-1] + 0.3 * P["rng"].standard_normal(gt[-1].shape)).astype(F32)
    args = (gt[0], P["onehot"], P["ef_raw"], gt, 0.0, t_at(4), SDT, 5)
    kw = dict(dt=SDT, adaptive=False, val_mask=vm, loss_scale=ns, cont_target=ct, cont_weight=0.02, want_pred=True)
    gs0, loss0, st0 = eng.solver_grad_tsit5(*args, **kw)
    gs2, loss2, st2 = eng.solver_grad_tsit5(*args, dense_saves=True, **kw)
    assert all(hit for _, _, hit in plan_of(st2, 0.0, t_at(4), 5))
    assert np.array_equal(st2["step_t"], st0["step_t"]) and np.array_equal(st2["step_h"], st0["step_h"])
    assert loss2 == loss0 and np.array_equal(gs2, gs0) and np.array_equal(st2["pred"], st0["pred"])
    assert (st2["n_accept"], st2["n_rhs"]) == (st0["n_accept"], st0["n_rhs"])


# The ground truth of the hidden_layers = 3 case is drawn with seed 9, not the fixture's 6, chosen by the one-ulp experiment that
# tests/test_gpu_group_solver_train.py documents (FIXED_SEED): the ReLUs make the gradient discontinuous at float32 resolution, and with
# seed 6 a pre-activation of the deeper network sits next to zero.  Measured on the MI355X, gradient rel-L2, this case's call:
#   the HOST composition's own gradient when x0 moves by one ulp up / down, nothing else:
#     hidden_layers 3: seed 6: 3.0e-4 / 3.0e-4, 7: 2.9e-5 / 7.5e-4, 8: 2.8e-5 / 1.0e-6, 9: 8.5e-7 / 7.7e-7, 10: 9.4e-7 / 1.5e-4
#     hidden_layers 1: seed 6: 5.6e-7 / 5.6e-7 (kept)
#   seed 6, hidden_layers 3: native against host 2.5e-4, against the moved hosts 6.6e-5, against the float64 oracle 6.4e-5 (the host
#   composition against the oracle: 3.0e-4) -- one flipped ReLU derivative in the host composition, not the interpolation.
# Seed 9 is the one seed whose host composition is stable in both directions; the tolerance stays the project's 1e-4.
@pytest.mark.parametrize("hidden_layers,ln_dims,seed", [(1, 0, 6), (3, 0, 9), (2, 1, 6)])
def test_hidden_layers_and_ln_all_against_host_composition(hidden_layers, ln_dims, seed):
    """dt = 0.025 to t1 = 0.04: saves 1, 2 inside the first step, the second cut to 0.015 with save 3 inside it"""
    P = problem(hidden_layers=hidden_layers, ln_dims=ln_dims, seed=seed)
    eng, gt, vm, ns = P["eng"], P["gt"], P["vm"], P["ns"]
    t1 = t_at(4)
    gs, loss, st = eng.solver_grad_tsit5(gt[0], P["onehot"], P["ef_raw"], gt, 0.0, t1, SDT, 5, dt=0.025, adaptive=False, dense_saves=True,
                                         val_mask=vm, loss_scale=ns)
    plan = plan_of(st, 0.0, t1, 5)
    assert [(i, hit) for i, _, hit in plan] == [(0, True), (0, False), (0, False), (1, False), (2, True)]
    rhs, vjp = host_fns(P)
    gs_h, loss_h, _, _, _ = tdr.tsit5_dense_adjoint(rhs, vjp, gt[0], gt, st["step_t"], st["step_h"], t1, plan, SDT, val_mask=vm, loss_scale=ns)
    print("hidden_layers %d ln_dims %d: host composition: loss %.2e gradient %.2e"
          % (hidden_layers, ln_dims, abs(loss - loss_h) / abs(loss_h), rel_l2(gs, gs_h)))
    assert abs(loss - loss_h) <= 1e-5 * abs(loss_h), (loss, loss_h)
    assert rel_l2(gs, gs_h) <= 1e-4, rel_l2(gs, gs_h)


def test_renumbered_graph_and_device_tensors():
    K = 5
    P = problem(K=K, scramble=True, n_points=400)
    eng, gt, vm, ns = P["eng"], P["gt"], P["vm"], P["ns"]
    assert renumbered(eng)
    ct = (gt[-1] + 0.3 * P["rng"].standard_normal(gt[-1].shape)).astype(F32)
    t1 = t_at(K)
    kw = dict(dt=0.025, adaptive=False, dense_saves=True, val_mask=vm, loss_scale=ns, cont_weight=0.02, want_pred=True)
    dev = torch.device("cuda", 0)
    gt_t, ct_t = torch.from_numpy(gt).to(dev), torch.from_numpy(ct).to(dev)
    out_t = torch.full((eng.param_count,), float("nan"), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    _, loss, st = eng.solver_grad_tsit5(gt[0], P["onehot"], P["ef_raw"], gt_t, 0.0, t1, SDT, K + 1, cont_target=ct_t, out=out_t, **kw)
    gs = out_t.cpu().numpy()
    gs_n, loss_n, st_n = eng.solver_grad_tsit5(gt[0], P["onehot"], P["ef_raw"], gt, 0.0, t1, SDT, K + 1, cont_target=ct, **kw)
    assert loss == loss_n and np.array_equal(gs, gs_n) and np.array_equal(st["pred"], st_n["pred"])
    plan = plan_of(st, 0.0, t1, K + 1)
    assert sum(not hit for _, _, hit in plan) == 4
    rhs, vjp = host_fns(P)
    gs_h, loss_h, pred_h, _, _ = tdr.tsit5_dense_adjoint(rhs, vjp, gt[0], gt, st["step_t"], st["step_h"], t1, plan, SDT, val_mask=vm,
                                                         loss_scale=ns, cont_target=ct, cont_weight=0.02)
    print("renumbered: host composition: loss %.2e gradient %.2e" % (abs(loss - loss_h) / abs(loss_h), rel_l2(gs, gs_h)))
    assert abs(loss - loss_h) <= 1e-5 * abs(loss_h), (loss, loss_h)
    assert rel_l2(gs, gs_h) <= 1e-4, rel_l2(gs, gs_h)
    assert rel_max(st["pred"], pred_h) <= 1e-5


def test_store_limit_step_record_and_refusals():
    P = problem(K=4)
    eng, gt = P["eng"], P["gt"]
    args = (gt[0], P["onehot"], P["ef_raw"], gt, 0.0, t_at(4), SDT, 5)
    kw = dict(dt=0.025, adaptive=False, dense_saves=True)
    stepb, denseb = 6 * P["N"] * 2 * 4, 7 * P["N"] * 2 * 4
    gs, loss, st = eng.solver_grad_tsit5(*args, **kw)
    assert st["n_steps"] == 2 and st["stored_bytes"] == 2 * stepb + denseb          # the sums of the interpolated saves are counted
    with pytest.raises(MgnError) as ei:
        eng.solver_grad_tsit5(*args, max_store_bytes=2 * stepb + denseb - 1, **kw)
    assert ei.value.code == _capi.MGN_E_OOM and "step 1" in str(ei.value) and "interpolated" in str(ei.value)
    with pytest.raises(MgnError) as ei:                                             # what the tstops modes need for two steps is not enough
        eng.solver_grad_tsit5(*args, max_store_bytes=2 * stepb, **kw)
    assert ei.value.code == _capi.MGN_E_OOM
    gs1, loss1, st1 = eng.solver_grad_tsit5(*args, max_store_bytes=2 * stepb + denseb, **kw)      # the handle still works
    assert loss1 == loss and np.array_equal(gs1, gs) and st1["stored_bytes"] == 2 * stepb + denseb
    gs2, loss2, st2 = eng.solver_grad_tsit5(*args, step_cap=1, **kw)
    assert st2["n_steps"] == 2 and len(st2["step_h"]) == 1 and np.array_equal(st2["step_t"], st["step_t"][:1])
    assert loss2 == loss and np.array_equal(gs2, gs)
    with pytest.raises(MgnError) as ei:                                             # the sixth save (t = 0.05) is beyond t1
        eng.solver_grad_tsit5(gt[0], P["onehot"], P["ef_raw"], np.concatenate([gt, gt[:1]]), 0.0, t_at(4), SDT, 6, **kw)
    assert ei.value.code == _capi.MGN_E_ARG and "reached" in str(ei.value)
    with pytest.raises(MgnError) as ei:
        eng.solver_grad_tsit5(*args, dt=0.0, adaptive=False, dense_saves=True)          # fixed steps need dt > 0
    assert ei.value.code == _capi.MGN_E_ARG
    # any other bit of the step mode
    d = _capi.MgnRolloutDesc()
    d.solver, d.t0, d.t1, d.dt, d.saves_dt, d.n_saves = 1, 0.0, t_at(4), 0.025, SDT, 5
    d.x0, d.node_type_onehot, d.ef_raw = _capi.f32(gt[0]), _capi.f32(P["onehot"]), _capi.f32(P["ef_raw"])
    g = np.zeros(eng.param_count, F32)
    lv = C.c_float()
    for mode in (4, 8, 6):
        o = _capi.MgnSolverGradOpts()
        o.adaptive = mode
        rc = eng.lib.mgn_solver_grad_tsit5(eng.h, C.byref(d), C.byref(o), _capi.f32(gt), None, None, 0.0, _capi.f32(g), g.size, C.byref(lv))
        assert rc == _capi.MGN_E_ARG, mode
    gs3, loss3, _ = eng.solver_grad_tsit5(*args, **kw)
    assert loss3 == loss and np.array_equal(gs3, gs)
    # reference_api: train_step(::MultipleShooting) as the reference solves it, window by window
    gsm, lossm = ra.train_step_multiple_shooting(eng, gt, P["onehot"], P["ef_raw"], 0.0, SDT, t_at(4), interval_size=3, continuity_term=100,
                                                 val_mask=P["vm"], solver="Tsit5", interpolate_saves=True)
    gsd, lossd = 0.0, 0.0
    for i, (a, b) in enumerate(ra.multiple_shooting_ranges(5, 3)):
        nxt = gt[b] if b < 4 else None
        gw, lw, _ = eng.solver_grad_tsit5(gt[a], P["onehot"], P["ef_raw"], gt[a:b + 1], ra._range_at(0.0, SDT, a, F32),
                                          ra._range_at(0.0, SDT, b, F32), SDT, b - a + 1, val_mask=P["vm"], cont_target=nxt,
                                          cont_weight=100.0 if nxt is not None else 0.0, dense_saves=True)
        gsd, lossd = gsd + gw.astype(np.float64), lossd + lw
    assert abs(lossm - lossd) <= 1e-6 * abs(lossd) and np.array_equal(gsm, gsd)
