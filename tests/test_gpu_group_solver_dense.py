"""mgn_group_solver_grad_tsit5 with MGN_TSIT5_DENSE_SAVES (GroupEngine.solver_grad_tsit5(dense_saves=True)) with P ranks on device 0:
every rank integrates, interpolates and sweeps the rows it owns; the loss divisor is the whole mesh's and the per-save loss partials go
through the group's rank-ordered fold.  The fixed-step case against one partition (the project's 1e-5 / 1e-4 between two summation orders,
ground truth drawn with seed 10 -- see FIXED_SEED in tests/test_gpu_group_solver_train.py), the adaptive case against the float64 oracle
over the group's OWN recorded steps (a group's step record and one partition's differ at small reltol, as documented there, so their
bits are not compared).  Fixture: tests/group_solver_case.py.  Run on the MI355X box with `-m gpu`.

Measured on the MI355X, gradient rel-L2: fixed steps against one partition 5.3e-7 (P = 2, val_mask + loss_scale) and 3.4e-5 (P = 3, inflow),
the losses bit for bit; adaptive against the oracle 1.3e-5 (P = 2, 6 accepted steps) and 8.4e-5 (P = 3, 7 accepted steps), saves 1 .. 5
interpolated in both."""
import ctypes as C

import numpy as np
import pytest
import torch   # noqa: F401  (before the engine's first HIP call)

import tsit5_dense_ref as tdr
from group_solver_case import case, oracle_fns
from mgn_amd import MgnError, _capi
from test_gpu_group_solver_train import FIXED_SEED, TOL_GS_ONE, TOL_LOSS_ONE, assert_partitioned, group, one, same_bits
from test_gpu_partitioned_step import rel_l2
from test_gpu_solver_train_tsit5_dense import ADAPTIVE_RELTOL, SDT, plan_of, t_at
from util import rel_max

pytestmark = pytest.mark.gpu

F32 = np.float32


@pytest.mark.parametrize("P,name", [pytest.param(2, "mask-scale", id="P2-mask-scale"), pytest.param(3, "inflow", id="P3-inflow")])
def test_fixed_steps_across_the_saves_against_one_partition(P, name):
    """dt = 0.025 over six saves of 0.01: saves 1, 2 inside the first step, 3, 4 inside the last, save 5 is x_K"""
    K = 5
    pr, e = case(K=K, seed=FIXED_SEED), one(K=K, seed=FIXED_SEED)
    gt = pr["gt"]
    kw = dict(val_mask=pr["vm"], loss_scale=pr["ns"])
    if name == "inflow":
        kw.update(inflow_mask=pr["inflow_mask"], inflow_data=pr["frames"])
    args = (gt[0], pr["onehot"], pr["ef_raw"], gt, 0.0, t_at(K), SDT, K + 1)
    mode = dict(dt=0.025, adaptive=False, dense_saves=True, want_pred=True)
    gs1, loss1, st1 = e.solver_grad_tsit5(*args, **mode, **kw)
    with group(pr, P) as g:
        views = assert_partitioned(g, pr, P)
        gs, loss, st = g.solver_grad_tsit5(*args, **mode, **kw)
        gs2, loss2, st2 = g.solver_grad_tsit5(*args, **mode, **kw)
        n_own0 = views[0].n_own
    assert loss2 == loss and same_bits(gs2, gs) and same_bits(st2["pred"], st["pred"])           # the same bits on two calls
    assert st["n_steps"] == 2 and same_bits(st["step_h"], st1["step_h"]) and same_bits(st["step_t"], st1["step_t"])
    assert st["stored_bytes"] == (2 * 6 + 7) * n_own0 * 2 * 4                                  # rank 0's own: memory is per rank
    plan = plan_of(st, 0.0, t_at(K), K + 1)
    assert [(i, hit) for i, _, hit in plan] == [(0, True), (0, False), (0, False), (1, False), (1, False), (2, True)]
    print("one partition: loss %.2e gradient %.2e pred %.2e" % (abs(loss - loss1) / abs(loss1), rel_l2(gs, gs1), rel_max(st["pred"], st1["pred"])))
    assert abs(loss - loss1) <= TOL_LOSS_ONE * abs(loss1), (loss, loss1)
    assert rel_l2(gs, gs1) <= TOL_GS_ONE, rel_l2(gs, gs1)
    assert rel_max(st["pred"], st1["pred"]) <= 1e-5


@pytest.mark.parametrize("P", [2, 3])
def test_adaptive_free_steps_against_the_oracle_over_the_groups_own_steps(P):
    K = 6
    pr = case(K=K)
    gt, vm, ns = pr["gt"], pr["vm"], pr["ns"]
    t1 = t_at(K)
    args = (gt[0], pr["onehot"], pr["ef_raw"], gt, 0.0, t1, SDT, K + 1)
    kw = dict(val_mask=vm, loss_scale=ns, abstol=1e-6, reltol=ADAPTIVE_RELTOL, dense_saves=True, want_pred=True)
    with group(pr, P) as g:
        assert_partitioned(g, pr, P)
        gs, loss, st = g.solver_grad_tsit5(*args, **kw)
        gs2, loss2, st2 = g.solver_grad_tsit5(*args, **kw)
    assert loss2 == loss and same_bits(gs2, gs) and same_bits(st2["pred"], st["pred"]) and same_bits(st2["step_h"], st["step_h"])
    plan = plan_of(st, 0.0, t1, K + 1)
    print("accepted steps %d, plan %s" % (st["n_accept"], plan))
    assert any(not hit for _, _, hit in plan) and plan[-1] == (st["n_steps"], None, True)
    rhs, vjp, _ = oracle_fns(pr)
    gs_o, loss_o, pred_o, _, _ = tdr.tsit5_dense_adjoint(rhs, vjp, gt[0], gt, st["step_t"], st["step_h"], t1, plan, SDT, val_mask=vm,
                                                         loss_scale=ns)
    print("oracle: loss %.2e gradient %.2e pred %.2e" % (abs(loss - loss_o) / abs(loss_o), rel_l2(gs, gs_o), rel_max(st["pred"], pred_o)))
    assert abs(loss - loss_o) <= 1e-4 * abs(loss_o), (loss, loss_o)
    assert rel_l2(gs, gs_o) <= 5e-3, rel_l2(gs, gs_o)
    assert rel_max(st["pred"], pred_o) <= 1e-4


def test_refusals_come_back_from_every_rank_and_leave_the_group_usable():
    pr = case()
    gt, oh, ef = pr["gt"], pr["onehot"], pr["ef_raw"]
    args = (gt[0], oh, ef, gt, 0.0, t_at(4), SDT, 5)
    mode = dict(dt=0.025, adaptive=False, dense_saves=True, val_mask=pr["vm"])
    with group(pr, 2) as g:
        assert_partitioned(g, pr, 2)
        before = g.solver_grad_tsit5(*args, **mode)
        d = _capi.MgnRolloutDesc()
        d.solver, d.t0, d.t1, d.dt, d.saves_dt, d.n_saves = 1, 0.0, t_at(4), 0.025, SDT, 5
        d.x0, d.node_type_onehot, d.ef_raw = _capi.f32(gt[0]), _capi.f32(oh), _capi.f32(ef)
        gs, lv = np.zeros(g.param_count, F32), C.c_float()
        for bad in (4, 8):
            o = _capi.MgnSolverGradOpts()
            o.adaptive = bad
            rc = g.lib.mgn_group_solver_grad_tsit5(g.g, C.byref(d), C.byref(o), _capi.f32(gt), None, None, 0.0, _capi.f32(gs), gs.size, C.byref(lv))
            assert rc == _capi.MGN_E_ARG and "rank" in g.lib.mgn_group_last_error(g.g).decode(), bad
        with pytest.raises(MgnError) as ei:                  # the sixth save (t = 0.05) is beyond t1
            g.solver_grad_tsit5(gt[0], oh, ef, np.concatenate([gt, gt[:1]]), 0.0, t_at(4), SDT, 6, **mode)
        assert ei.value.code == _capi.MGN_E_ARG and "rank" in str(ei.value) and "reached" in str(ei.value)
        with pytest.raises(MgnError) as ei:                  # fixed steps need dt > 0
            g.solver_grad_tsit5(*args, **dict(mode, dt=0.0))
        assert ei.value.code == _capi.MGN_E_ARG and "rank" in str(ei.value)
        after = g.solver_grad_tsit5(*args, **mode)
        assert after[1] == before[1] and same_bits(after[0], before[0])
