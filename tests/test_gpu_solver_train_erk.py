"""mgn_solver_grad_erk (Engine.solver_grad_erk): the loss and discrete-adjoint gradient of one fixed-step solve with an explicit
Runge-Kutta tableau on the device, against mgn_solver_grad_tsit5 bit for bit for the Tsit5 tableau (the same loop and the same
table-driven sweep, handed the same coefficients) and against mgn_solver_grad bit for bit for the Euler tableau, against tests/erk_ref.py's erk_adjoint composed from mgn_ode_step / mgn_ode_vjp on
the same engine and from the float64 oracle, and against Engine.rollout's solution.  Fixtures: test_gpu_solver_train.problem (the
150-point cylinder, L = 64, mps = 2, K = 4 steps of 0.01), and 151 points where N * O is no multiple of four (the stage-seed kernel's
scalar form).  Tolerances: those of tests/test_gpu_solver_train_tsit5.py's fixed-step cases.  Run on the MI355X with `-m gpu`.

Measured on the MI355X, gradient rel L2 against the host composition (bound 1e-4) / the float64 oracle (bound 5e-3); the losses agree
to 2e-7 relative: RK4 1.1e-7 / 1.4e-6, Heun at half steps 1.2e-7 / 9.1e-8, BS3 1.5e-7 / 1.1e-7, DP5 1.8e-7 / 1.5e-4 (151 points:
9.3e-6 / 6.1e-6), Euler 9.4e-8 / 1.4e-7; with the inflow mask and the continuity term against the oracle: RK4 8.5e-6, BS3 5.7e-8."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch   # noqa: F401  (before the engine's first HIP call)

import erk_ref
from mgn_amd import MgnError, _capi, erk_tableau
from test_gpu_group_solver_train import same_bits
from test_gpu_solver_train import eng_fns, oracle_fns, problem, rel_l2

pytestmark = pytest.mark.gpu

F32 = np.float32
SDT, K = 0.01, 4
T1 = float(F32(K * SDT))
ACTIVE = dict(Euler=1, Heun=2, RK4=4, BS3=3, DP5=6, Tsit5=6)       # s' = s - fsal


@functools.lru_cache(maxsize=None)
def prob(**kw):
    """this module's own problem, made once per shape"""
    return problem(K=K, **kw)


def inflow_of(P, seed=21):
    im = ((P["node_type"] == 4) | (P["node_type"] == 1)).astype(np.uint8)
    assert im.any() and not im.all()
    frames = (P["gt"][0][None] * (1.0 + 0.2 * np.random.default_rng(seed).standard_normal((K + 2, P["N"], 2)))).astype(F32)
    return im, frames


def grad(eng, P, tab, dt=SDT, **kw):
    gt = P["gt"]
    return eng.solver_grad_erk(tab, gt[0], P["onehot"], P["ef_raw"], gt, 0.0, T1, SDT, K + 1, dt, val_mask=P["vm"], **kw)


# ---- C.1: the Tsit5 tableau is mgn_solver_grad_tsit5 in step mode 0 ---------------------------------------------------------------------
@pytest.mark.parametrize("n_points,factor", [(150, 1.0), (150, 0.5), (151, 1.0)])
def test_tsit5_tableau_returns_the_bits_of_solver_grad_tsit5(n_points, factor):
    P = prob(n_points=n_points)
    eng, gt = P["eng"], P["gt"]
    im, frames = inflow_of(P)
    ct = (gt[-1] + 0.3 * np.random.default_rng(5).standard_normal(gt[-1].shape)).astype(F32)
    kw = dict(inflow_mask=im, inflow_data=frames, loss_scale=P["ns"], cont_target=ct, cont_weight=0.01, want_pred=True)
    gs_r, loss_r, st_r = eng.solver_grad_tsit5(gt[0], P["onehot"], P["ef_raw"], gt, 0.0, T1, SDT, K + 1, dt=factor * SDT, adaptive=False,
                                               val_mask=P["vm"], **kw)
    gs, loss, st = grad(eng, P, erk_tableau("Tsit5"), factor * SDT, **kw)
    assert np.float32(loss).tobytes() == np.float32(loss_r).tobytes() and same_bits(gs, gs_r) and same_bits(st["pred"], st_r["pred"])
    assert same_bits(st["step_t"], st_r["step_t"]) and same_bits(st["step_h"], st_r["step_h"]) and len(st["step_h"]) == int(K / factor)
    for key in ("n_accept", "n_reject", "n_rhs", "n_steps", "stored_bytes"):
        assert st[key] == st_r[key], key
    assert np.abs(gs).max() > 0 and np.isfinite(gs).all()


@pytest.mark.parametrize("factor,inflow,full", [(1, False, False), (2, False, False), (1, True, False), (2, True, False), (2, True, True)])
def test_euler_tableau_returns_the_bits_of_solver_grad(factor, inflow, full):
    """two save intervals of 2 / factor steps each (K = 2 and 4); full: loss_scale, val_mask and the continuity term as well.  The two
    entry points differ in their checks and in what they ask of the handle, not in a bit of what they return"""
    P = prob()
    eng, gt = P["eng"], P["gt"][:3]
    t1, dt = float(F32(2 * SDT)), SDT / factor
    kw = dict(want_pred=True)
    if inflow:
        kw["inflow_mask"], kw["inflow_data"] = inflow_of(P)
    if full:
        ct = (gt[-1] + 0.3 * np.random.default_rng(5).standard_normal(gt[-1].shape)).astype(F32)
        kw.update(val_mask=P["vm"], loss_scale=P["ns"], cont_target=ct, cont_weight=0.01)
    gs_r, loss_r, pred_r = eng.solver_grad(gt[0], P["onehot"], P["ef_raw"], gt, 0.0, t1, dt, SDT, 3, **kw)
    gs, loss, st = eng.solver_grad_erk(erk_tableau("Euler"), gt[0], P["onehot"], P["ef_raw"], gt, 0.0, t1, SDT, 3, dt, **kw)
    assert np.float32(loss).tobytes() == np.float32(loss_r).tobytes() and same_bits(gs, gs_r) and same_bits(st["pred"], pred_r)
    assert (st["n_accept"], st["n_reject"], st["n_rhs"], st["n_steps"]) == (2 * factor, 0, 2 * factor, 2 * factor)
    assert np.abs(gs).max() > 0 and np.isfinite(gs).all() and loss > 0


# ---- C.2: the other methods against the host composition and the float64 oracle -------------------------------------------------------
CASES = [pytest.param("RK4", 150, 1.0, id="RK4"), pytest.param("Heun", 150, 0.5, id="Heun-half-steps"), pytest.param("BS3", 150, 1.0, id="BS3"),
         pytest.param("DP5", 150, 1.0, id="DP5"), pytest.param("DP5", 151, 1.0, id="DP5-151-points"), pytest.param("Euler", 150, 1.0, id="Euler")]


@pytest.mark.parametrize("name,n_points,factor", CASES)
def test_against_host_composition_oracle_and_rollout(name, n_points, factor):
    P = prob(n_points=n_points)
    eng, gt, vm, ns = P["eng"], P["gt"], P["vm"], P["ns"]
    tab = erk_tableau(name)
    dt, steps = factor * SDT, int(K / factor)
    gs, loss, st = grad(eng, P, tab, dt, loss_scale=ns, want_pred=True)
    sp = ACTIVE[name]
    assert (st["n_accept"], st["n_reject"], st["n_steps"]) == (steps, 0, steps)
    assert st["n_rhs"] == (1 + sp * steps if tab.fsal else sp * steps) and st["stored_bytes"] == steps * sp * P["N"] * 2 * 4
    sol, rst = eng.rollout(tab, gt[0], P["onehot"], P["ef_raw"], 0.0, T1, SDT, K + 1, dt=dt, adaptive=False, val_mask=vm)
    assert same_bits(st["pred"], sol) and rst["n_rhs"] == st["n_rhs"]       # no inflow mask: the same launches
    a = (tab, gt[0], gt, 0.0, T1, dt, SDT, K + 1)
    rhs, vjp = eng_fns(P)
    gs_h, loss_h, _ = erk_ref.erk_adjoint(rhs, vjp, *a, val_mask=vm, loss_scale=ns)
    o_rhs, o_vjp, _ = oracle_fns(P)
    gs_o, loss_o, pred_o = erk_ref.erk_adjoint(o_rhs, o_vjp, *a, val_mask=vm, loss_scale=ns)
    print("%s, %d points: loss %.6e (host composition %.6e, oracle %.6e); gradient rel L2 %.3e against the host composition, %.3e against "
          "the oracle" % (name, n_points, loss, loss_h, loss_o, rel_l2(gs, gs_h), rel_l2(gs, gs_o)))
    assert abs(loss - loss_h) <= 1e-4 * abs(loss_h) and abs(loss - loss_o) <= 1e-4 * abs(loss_o)
    assert rel_l2(gs, gs_h) <= 1e-4
    assert rel_l2(gs, gs_o) <= 5e-3
    if name == "Euler":       # one stage: Euler's own entry point computes the same thing
        gs_e, loss_e = eng.solver_grad(gt[0], P["onehot"], P["ef_raw"], gt, 0.0, T1, dt, SDT, K + 1, val_mask=vm, loss_scale=ns)
        assert abs(loss - loss_e) <= 1e-6 * abs(loss_e) and rel_l2(gs, gs_e) <= 1e-4


@pytest.mark.parametrize("name", ["RK4", "BS3"])
def test_inflow_copies_and_continuity_term_against_the_oracle(name):
    """the training form: the right-hand sides see copies with the inflow rows of their stage's frame (dt = saves_dt / 2: the stages of
    a step read one frame, consecutive steps of a save period too, the FSAL evaluation the next), the state is never overwritten"""
    P = prob()
    eng, gt, vm, ns = P["eng"], P["gt"], P["vm"], P["ns"]
    tab = erk_tableau(name)
    im, frames = inflow_of(P)
    ct = (gt[-1] + 0.3 * np.random.default_rng(5).standard_normal(gt[-1].shape)).astype(F32)
    kw = dict(val_mask=vm, inflow_mask=im, inflow_data=frames, loss_scale=ns, cont_target=ct, cont_weight=0.01)
    gs, loss, st = grad(eng, P, tab, 0.5 * SDT, want_pred=True, **{k: v for k, v in kw.items() if k != "val_mask"})
    o_rhs, o_vjp, o_rhs_at = oracle_fns(P, inflow_mask=im.astype(bool), frames=frames)
    gs_o, loss_o, pred_o = erk_ref.erk_adjoint(o_rhs, o_vjp, tab, gt[0], gt, 0.0, T1, 0.5 * SDT, SDT, K + 1, rhs_at=o_rhs_at, **kw)
    print("%s with the inflow mask: loss %.6e (oracle %.6e), gradient rel L2 %.3e" % (name, loss, loss_o, rel_l2(gs, gs_o)))
    assert abs(loss - loss_o) <= 1e-4 * abs(loss_o)
    assert rel_l2(gs, gs_o) <= 5e-3
    assert np.abs(st["pred"] - pred_o).max() <= 1e-4 * np.abs(pred_o).max()
    assert same_bits(st["pred"][0], gt[0])                                       # the state is not overwritten
    again = grad(eng, P, tab, 0.5 * SDT, want_pred=True, **{k: v for k, v in kw.items() if k != "val_mask"})
    assert same_bits(again[0], gs) and again[1] == loss                          # repeatable


def test_reference_api_training_helpers_take_the_new_names():
    """train_step_solver_training / train_step_multiple_shooting with solver="RK4": Engine.solver_grad_erk window by window"""
    from mgn_amd import reference_api as ra
    P = prob()
    eng, gt, vm, ns = P["eng"], P["gt"], P["vm"], P["ns"]
    gs, loss, _ = grad(eng, P, "RK4", loss_scale=ns)
    gs_r, loss_r = ra.train_step_solver_training(eng, gt, P["onehot"], P["ef_raw"], 0.0, SDT, T1, val_mask=vm, n_scale=ns, solver="RK4")
    assert same_bits(gs_r, gs) and loss_r == loss
    gs_t, loss_t = ra.train_step_solver_training(eng, gt, P["onehot"], P["ef_raw"], 0.0, SDT, T1, val_mask=vm, n_scale=ns,
                                                 solver=erk_tableau("RK4"), adaptive=False)
    assert same_bits(gs_t, gs) and loss_t == loss
    gs_m, loss_m = ra.train_step_multiple_shooting(eng, gt, P["onehot"], P["ef_raw"], 0.0, SDT, T1, 3, 0.01, val_mask=vm, solver="BS3")
    assert np.isfinite(gs_m).all() and np.abs(gs_m).max() > 0 and loss_m > 0
    w0 = eng.solver_grad_erk("BS3", gt[0], P["onehot"], P["ef_raw"], gt[0:3], 0.0, float(F32(2 * SDT)), SDT, 3, SDT, val_mask=vm,
                             cont_target=gt[2], cont_weight=0.01)
    w1 = eng.solver_grad_erk("BS3", gt[2], P["onehot"], P["ef_raw"], gt[2:5], float(F32(2 * SDT)), T1, SDT, 3, SDT, val_mask=vm)
    assert abs(loss_m - (w0[1] + w1[1])) <= 1e-6 * loss_m and rel_l2(gs_m, w0[0].astype(np.float64) + w1[0]) <= 1e-6
    with pytest.raises(ValueError):
        ra.train_step_multiple_shooting(eng, gt, P["onehot"], P["ef_raw"], 0.0, SDT, T1, 3, 0.01, val_mask=vm, solver="BS3", batched=True)
    with pytest.raises(ValueError):
        ra.train_step_solver_training(eng, gt, P["onehot"], P["ef_raw"], 0.0, SDT, T1, val_mask=vm, solver="RK45")


# ---- C.3: refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable():
    P = prob()
    eng, gt = P["eng"], P["gt"]
    rk4 = erk_tableau("RK4")
    before = grad(eng, P, rk4)

    def still_works():
        again = grad(eng, P, rk4)
        assert same_bits(again[0], before[0]) and again[1] == before[1]

    def code_of(call):
        with pytest.raises(MgnError) as ei:
            call()
        return ei.value.code

    d, keep, p_gt, ls, p_ct, gs, p_gs, pred = eng._solver_desc("Euler", gt[0], P["onehot"], P["ef_raw"], gt, 0.0, T1, SDT, SDT, K + 1, P["vm"],
                                                               None, None, None, None, "reference", F32, False, None)
    lv = C.c_float()

    def raw(tab_ptr, o):
        return eng.lib.mgn_solver_grad_erk(eng.h, C.byref(d), tab_ptr, C.byref(o) if o is not None else None, p_gt, None, None, 0.0, p_gs,
                                           eng.param_count, C.byref(lv))

    o = _capi.MgnSolverGradOpts()
    bad = rk4.tab.copy()
    bad[55] = 0.5                                                                # sum b != 1
    assert raw(bad.ctypes.data_as(C.POINTER(C.c_double)), o) == _capi.MGN_E_ARG
    assert raw(None, o) == _capi.MGN_E_ARG and raw(rk4._ptr(), None) == _capi.MGN_E_ARG
    for mode in (1, 2, 3):                                                       # fixed steps only
        o.adaptive = mode
        assert raw(rk4._ptr(), o) == _capi.MGN_E_UNSUPPORTED
        assert raw(erk_tableau("BS3")._ptr(), o) == _capi.MGN_E_UNSUPPORTED
    o.adaptive = 0
    dp5 = erk_tableau("DP5")
    seven = erk_tableau(dp5.A, dp5.b, dp5.c, order=5)                            # DP5 without the FSAL flag: seven active stages
    assert raw(seven._ptr(), o) == _capi.MGN_E_UNSUPPORTED
    still_works()
    assert code_of(lambda: grad(eng, P, rk4, 0.0)) == _capi.MGN_E_ARG
    assert code_of(lambda: grad(eng, P, rk4, -SDT)) == _capi.MGN_E_ARG
    assert code_of(lambda: grad(eng, P, rk4, SDT / 2.5)) == _capi.MGN_E_ARG      # saves_dt / dt = 2.5
    assert code_of(lambda: grad(eng, P, rk4, max_store_bytes=4 * P["N"] * 2 * 4)) == _capi.MGN_E_OOM      # one step's four stage inputs only
    still_works()
    d.solver = 3                                                                 # not read
    assert raw(rk4._ptr(), o) == _capi.MGN_OK
    assert same_bits(gs, before[0])
    del keep
    still_works()
