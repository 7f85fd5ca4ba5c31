"""mgn_rollout / mgn_rollout_eval and their group forms with MGN_SOLVER_TSIT5_FIXED (Engine.rollout("Tsit5", ..., adaptive=False)):
`solve(prob, Tsit5(); adaptive = false, dt, saveat = saves)` over ode_func_eval -- the time loop of step mode 2 of mgn_solver_grad_tsit5
with nothing stored, the inflow rows written in place by the fused stage-input kernel, every save reduced as it is produced.

References: the training form (Engine.solver_grad_tsit5(adaptive=False, dense_saves=True)), bit for bit where there is no inflow mask;
a host replay of the loop in NumPy float32 on the engine's own right-hand side (tests/tsit5_fixed_eval_ref.py); float64 NumPy reductions
of the saves; the coherent numbering; one partition.  Fixtures: the 150-point cylinder of tests/test_gpu_solver_train.py (L = 64,
mps = 2, at most ten steps), 151 points where the element count must not be a multiple of four (the kernel's scalar tail, and frames
that are not 16-byte aligned), and for the partitions the 1320-node grid of tests/group_solver_case.py, the one fixture in which every
rank of P = 2, 3 owns boundary rows, interior rows and a halo.  Run on the MI355X box with `-m gpu`.

Measured on the MI355X (every test prints its figures before it asserts), rel_max against the host replay, dt = 0.4 saves_dt, 10 steps:
  150 points: without a mask (the replay's own noise) 2.54e-7, with the inflow mask 2.54e-7 (bound: 4 x the noise = 1.0e-6)
  151 points: without a mask 2.30e-7, with the inflow mask 2.30e-7 (the largest deviation sits on a row outside the mask in all four)
  bf16 handle (L = 128) against the fp32 replay: relative L2 7.5e-4 (band 3e-2)
  renumbered (400 points) against the coherent numbering: relative L2 1.2e-7 (tolerance 1e-3)
  groups of 2 / 3 ranks against one partition: rel_max 1.8e-7 / 1.8e-7 (tolerance 1e-5)"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch   # noqa: F401  (before the engine's first HIP call)

import tsit5_dense_ref as tdr
import tsit5_fixed_eval_ref as fer
from group_solver_case import case
from mgn_amd import MgnError, _capi
from test_gpu_group_solver_train import TOL_FWD, assert_partitioned, check_reductions, group, one, same_bits
from test_gpu_solver_train import problem
from util import TOL_ROLLOUT, engine_for, rel_max, renumbered

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SDT = 0.01
TOL_BF16 = 3e-2      # relative L2, DESIGN.md section 2


@functools.lru_cache(maxsize=None)
def prob(**kw):
    """test_gpu_solver_train.problem, made once per shape and shared (its engine keeps no state between calls)"""
    return problem(**kw)


def t_at(i, time_type=F32):
    """save time i in the solver's time type, as the library forms it"""
    tt = np.dtype(time_type).type
    return float(tt(i * float(tt(SDT))))


def inflow_of(P, n_frames, seed=21):
    im = ((P["node_type"] == 4) | (P["node_type"] == 1)).astype(np.uint8)
    assert im.any() and not im.all()
    frames = (P["gt"][0][None] * (1.0 + 0.2 * np.random.default_rng(seed).standard_normal((n_frames, P["N"], 2)))).astype(F32)
    return im, frames


def fixed(eng, P, K, dt, x0=None, **kw):
    x0 = P["gt"][0] if x0 is None else x0
    tt = kw.get("time_type", F32)
    return eng.rollout("Tsit5", x0, P["onehot"], P["ef_raw"], 0.0, t_at(K, tt), SDT, K + 1, dt=dt, adaptive=False, val_mask=P["vm"], **kw)


def host_replay(eng, P, K, dt, **kw):
    """tests/tsit5_fixed_eval_ref.py on eng's resident right-hand side"""
    eng.set_static(P["onehot"], P["ef_raw"], P["vm"])
    tt = kw.get("time_type", F32)
    return fer.replay(lambda x: eng.ode_step(np.ascontiguousarray(x, F32)), P["gt"][0], 0.0, t_at(K, tt), dt, SDT, K + 1, **kw)


# ---- 1: pinned by the training form ------------------------------------------------------------------------------------------------------
CASES = [pytest.param(f, tt, dict(), id="dt%g-%s" % (f, np.dtype(tt).name)) for f in (1.0, 0.4, 2.5) for tt in (F32, F64)]
CASES += [pytest.param(0.4, F32, dict(ln_dims=1), id="dt0.4-ln_all"), pytest.param(2.5, F32, dict(n_points=151), id="dt2.5-151-points")]


@pytest.mark.parametrize("factor,time_type,shape", CASES)
def test_evaluation_form_returns_the_bits_of_the_training_form(factor, time_type, shape):
    """no inflow mask: the same launches.  dt = saves_dt: every save on a step end; 0.4 saves_dt: saves inside steps and on ends; 2.5
    saves_dt: several saves in one step, the last step cut to reach t1"""
    K = 4
    P = prob(K=K, **shape)
    eng, gt = P["eng"], P["gt"]
    dt, t1 = factor * SDT, t_at(K, time_type)
    sol, st = fixed(eng, P, K, dt, time_type=time_type)
    _, _, tr = eng.solver_grad_tsit5(gt[0], P["onehot"], P["ef_raw"], gt, 0.0, t1, SDT, K + 1, dt=dt, adaptive=False, dense_saves=True,
                                     val_mask=P["vm"], time_type=time_type, want_pred=True)
    step_t, step_h, t_end = tdr.fixed_dense_steps(0.0, t1, dt, SDT, time_type)
    print("steps", step_h, "plan", tdr.dense_plan(step_t, step_h, t_end, 0.0, SDT, K + 1, time_type))
    assert tr["step_t"].tolist() == step_t and tr["step_h"].tolist() == step_h and t_end == t1
    assert len(step_h) == {1.0: 4, 0.4: 10, 2.5: 2}[factor]
    if factor == 2.5:
        assert step_h[1] < step_h[0]
    assert st == dict(n_accept=tr["n_steps"], n_reject=0, n_rhs=1 + 6 * tr["n_steps"])
    assert (tr["n_accept"], tr["n_reject"], tr["n_rhs"]) == (st["n_accept"], 0, st["n_rhs"])
    assert same_bits(sol, tr["pred"])
    assert same_bits(sol[0], gt[0]) and np.isfinite(sol).all()
    sol2, st2 = fixed(eng, P, K, dt, time_type=time_type)                     # abstol / reltol are ignored; the same bits on a second call
    sol3, _ = fixed(eng, P, K, dt, time_type=time_type, abstol=0.0, reltol=-1.0)
    assert same_bits(sol2, sol) and st2 == st and same_bits(sol3, sol)


# ---- 2: the in-place inflow overwrite ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_points", [150, 151])
def test_inflow_rows_are_written_in_place(n_points):
    """dt = 0.4 saves_dt over four save periods: the stages of a step read different frames.  The tolerance against the host replay is
    measured: four times the replay's own distance from the native result on the run without a mask, which test 1 pins.  Measured on
    the MI355X, rel_max: 150 points 2.54e-7 without / 2.54e-7 with the mask; 151 points 2.30e-7 / 2.30e-7."""
    K, dt = 4, 0.4 * SDT
    P = prob(K=K, n_points=n_points)
    eng, gt = P["eng"], P["gt"]
    im, frames = inflow_of(P, K + 2)
    m = im.astype(bool)
    plain, _ = fixed(eng, P, K, dt)
    sol, st = fixed(eng, P, K, dt, inflow_mask=im, inflow_data=frames, inflow_rule="reference")
    assert same_bits(sol[0], gt[0])                                           # taken before the first right-hand side
    ref, step_t, step_h, plan, rst = host_replay(eng, P, K, dt, inflow_mask=im, inflow_data=frames)
    assert st == rst
    times = list(step_t) + [t_at(K)]
    sdt = float(F32(SDT))
    on_ends = [(s, idx) for s, (idx, _, hit) in enumerate(plan) if hit and idx > 0]
    assert on_ends and any(not hit for _, _, hit in plan)
    for s, idx in on_ends:
        fr = int(np.floor(F32(F32(times[idx]) / F32(sdt))))
        assert same_bits(sol[s][m], frames[fr][m]), (s, idx, fr)
    assert not np.array_equal(sol[1:, ~m], plain[1:, ~m])
    ref0 = host_replay(eng, P, K, dt)[0]
    noise, err = rel_max(plain, ref0), rel_max(sol, ref)
    print("%d points: host replay: without a mask %.3e, with the inflow mask %.3e" % (n_points, noise, err))
    assert 0.0 < noise <= 1e-5
    assert err <= 4.0 * noise, (err, noise)


# ---- 3: rollout_eval -----------------------------------------------------------------------------------------------------------------------
def test_rollout_eval_reduces_every_save_with_and_without_a_solution_buffer():
    K, dt = 4, 0.4 * SDT
    P = prob(K=K)
    eng, gt = P["eng"], P["gt"]
    x0 = (gt[0] * F32(1.02)).astype(F32)                                       # (not gt[0]: every save differs from its frame)
    im, _ = inflow_of(P, K + 1)
    sel = np.arange(3, 2 * P["N"], 7, dtype=np.int32)
    a = ("Tsit5", x0, P["onehot"], P["ef_raw"])
    k = dict(dt=dt, adaptive=False, val_mask=P["vm"])
    for ik in (dict(), dict(inflow_mask=im, inflow_data=gt, inflow_rule="tolerant")):
        sol, st = eng.rollout(*a, 0.0, t_at(K), SDT, K + 1, **k, **ik)
        plan = tdr.dense_plan(*tdr.fixed_dense_steps(0.0, t_at(K), dt, SDT), 0.0, SDT, K + 1)
        assert any(not hit for _, _, hit in plan)                              # interior saves pass through the reduction too
        for s_, b_ in ((None, 0), (sel, 0), (sel + 1, 1)):
            r = eng.rollout_eval(*a, gt, 0.0, t_at(K), SDT, K + 1, sel=s_, sel_index_base=b_, want_pred=True, **k, **ik)
            assert same_bits(r["pred"], sol) and r["stats"] == st
            check_reductions(r, r["pred"], gt, s_, b_)
            q = eng.rollout_eval(*a, gt, 0.0, t_at(K), SDT, K + 1, sel=s_, sel_index_base=b_, **k, **ik)      # no solution buffer
            assert q["pred"] is None and q["stats"] == st
            assert np.float64(q["val_loss"]).tobytes() == np.float64(r["val_loss"]).tobytes()
            assert same_bits(q["mse_save"], r["mse_save"]) and same_bits(q["mse_time"], r["mse_time"])
        if ik:                                                                 # gt IS the inflow data (one pointer), or a separate array
            one_ptr = eng.rollout_eval(*a, gt, 0.0, t_at(K), SDT, K + 1, **k, **ik)
            two = eng.rollout_eval(*a, gt.copy(), 0.0, t_at(K), SDT, K + 1, **k, **ik)
            assert np.float64(one_ptr["val_loss"]).tobytes() == np.float64(two["val_loss"]).tobytes()
            assert same_bits(one_ptr["mse_save"], two["mse_save"]) and same_bits(one_ptr["mse_time"], two["mse_time"])


# ---- 4: a renumbered handle ----------------------------------------------------------------------------------------------------------------
def test_renumbered_handle_agrees_with_the_coherent_numbering():
    """400 points under scattered labels (the engine renumbers) against the same mesh in its coherent numbering, in the caller's order"""
    K, dt = 4, 0.4 * SDT
    Pc, Ps = prob(K=K, n_points=400), prob(K=K, n_points=400, scramble=True)
    assert renumbered(Ps["eng"])
    perm = np.random.default_rng(3).permutation(Pc["N"]).astype(np.int32)     # util.scatter_labels(seed=3): perm[old] = new label
    inv = np.argsort(perm)
    assert np.array_equal(Ps["onehot"], Pc["onehot"][inv]) and np.array_equal(Ps["vm"], Pc["vm"][inv])
    im, frames = inflow_of(Pc, K + 2)
    x0 = Pc["gt"][0]
    ref, st_c = fixed(Pc["eng"], Pc, K, dt, x0=x0, inflow_mask=im, inflow_data=frames)
    sol, st_s = fixed(Ps["eng"], Ps, K, dt, x0=np.ascontiguousarray(x0[inv]), inflow_mask=np.ascontiguousarray(im[inv]),
                      inflow_data=np.ascontiguousarray(frames[:, inv]))
    back = sol[:, perm]
    err = float(np.linalg.norm(back.astype(F64) - ref) / np.linalg.norm(ref.astype(F64)))
    print("renumbered against coherent: relative L2 %.3e" % err)
    assert st_s == st_c
    assert err <= TOL_ROLLOUT
    assert same_bits(back[0], x0)


# ---- 5: partitions -------------------------------------------------------------------------------------------------------------------------
def group_args(pr, K):
    return ("Tsit5", pr["gt"][0], pr["onehot"], pr["ef_raw"], 0.0, t_at(K), SDT, K + 1)


def group_kw(pr):
    return dict(dt=0.4 * SDT, adaptive=False, val_mask=pr["vm"], inflow_mask=pr["inflow_mask"], inflow_data=pr["frames"])


def test_group_of_one_returns_the_bits_of_the_engine():
    pr, e = case(), one()
    ref, st1 = e.rollout(*group_args(pr, 4), **group_kw(pr))
    q = e.rollout_eval(*group_args(pr, 4)[:4], pr["gt"], *group_args(pr, 4)[4:], **group_kw(pr))
    with group(pr, 1) as g:
        sol, st = g.rollout(*group_args(pr, 4), **group_kw(pr))
        r = g.rollout_eval(*group_args(pr, 4)[:4], pr["gt"], *group_args(pr, 4)[4:], **group_kw(pr))
    assert same_bits(sol, ref) and st == st1 and st["n_accept"] == 10
    assert np.float64(r["val_loss"]).tobytes() == np.float64(q["val_loss"]).tobytes() and r["stats"] == q["stats"]
    assert same_bits(r["mse_save"], q["mse_save"]) and same_bits(r["mse_time"], q["mse_time"])


@pytest.mark.parametrize("P", [2, 3])
def test_groups_are_held_to_one_partition(P):
    """every rank integrates the rows it owns; no error norm, so nothing but the halo exchanges of the right-hand sides crosses ranks"""
    pr, e = case(), one()
    ref, st1 = e.rollout(*group_args(pr, 4), **group_kw(pr))
    with group(pr, P) as g:
        assert_partitioned(g, pr, P)
        sol, st = g.rollout(*group_args(pr, 4), **group_kw(pr))
        r = g.rollout_eval(*group_args(pr, 4)[:4], pr["gt"], *group_args(pr, 4)[4:], want_pred=True, **group_kw(pr))
        q = g.rollout_eval(*group_args(pr, 4)[:4], pr["gt"], *group_args(pr, 4)[4:], **group_kw(pr))
    print("P = %d against one partition: rel_max %.3e" % (P, rel_max(sol, ref)))
    assert st == st1 == dict(n_accept=10, n_reject=0, n_rhs=61)
    assert rel_max(sol, ref) <= TOL_FWD
    assert same_bits(r["pred"], sol) and r["stats"] == st
    check_reductions(r, r["pred"], pr["gt"])
    assert q["pred"] is None and np.float64(q["val_loss"]).tobytes() == np.float64(r["val_loss"]).tobytes()
    assert same_bits(q["mse_save"], r["mse_save"]) and same_bits(q["mse_time"], r["mse_time"])


# ---- 6: bf16 -------------------------------------------------------------------------------------------------------------------------------
def test_bf16_handle_against_the_host_replay():
    """the bf16 handle's rollout (L = 128: the bf16 mode's one shape) against the replay on the fp32 engine's right-hand side, at the
    project's bf16 band.  Measured on the MI355X: 7.5e-4 relative L2"""
    K, dt = 4, 0.4 * SDT
    P = prob(K=K, L=128)
    im, frames = inflow_of(P, K + 2)
    b = engine_for(P["cfg"], dtype="bf16")
    b.set_params(P["ps"])
    b.set_graph(P["s"], P["r"], P["N"])
    ns, ts, es = P["n_norm"].affine(2), P["t_norm"].affine(7), P["e_norm"].affine(3)
    b.set_norms(node=(np.concatenate([ns[0], ts[0]]), np.concatenate([ns[1], ts[1]])), edge=es, out=(P["o_norm"].std, P["o_norm"].mean))
    sol, st = fixed(b, P, K, dt, inflow_mask=im, inflow_data=frames)
    ref, _, _, _, rst = host_replay(P["eng"], P, K, dt, inflow_mask=im, inflow_data=frames)
    err = float(np.linalg.norm(sol.astype(F64) - ref) / np.linalg.norm(ref.astype(F64)))
    print("bf16: relative L2 against the fp32 replay %.3e" % err)
    assert st == rst
    assert 0.0 < err <= TOL_BF16
    b.close()


# ---- 7: refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable():
    K, dt = 4, 0.4 * SDT
    P = prob(K=K)
    eng, gt = P["eng"], P["gt"]
    before, st = fixed(eng, P, K, dt)

    def still_works():
        again, st2 = fixed(eng, P, K, dt)
        assert same_bits(again, before) and st2 == st

    for tt in (F32, F64):
        with pytest.raises(MgnError) as ei:                                    # fixed steps need dt > 0, in either time type
            fixed(eng, P, K, 0.0, time_type=tt)
        assert ei.value.code == _capi.MGN_E_ARG
        with pytest.raises(MgnError) as ei:
            fixed(eng, P, K, -dt, time_type=tt)
        assert ei.value.code == _capi.MGN_E_ARG
        still_works()
    d, keep = eng._rollout_desc("Tsit5", gt[0], P["onehot"], P["ef_raw"], 0.0, t_at(K), SDT, K + 1, dt, P["vm"], None, None, 1e-6, 1e-3,
                                "reference", F32, adaptive=False)
    assert d.solver == _capi.MGN_SOLVER_TSIT5_FIXED == 2
    out = np.zeros((K + 1, P["N"], 2), F32)
    d.out = _capi.f32(out)
    for bad in (3, -1):
        d.solver = bad
        assert eng.lib.mgn_rollout(eng.h, C.byref(d)) == _capi.MGN_E_ARG, bad
        ev = _capi.MgnRolloutEvalDesc()
        ev.gt, ev.n_gt = _capi.f32(gt), K + 1
        assert eng.lib.mgn_rollout_eval(eng.h, C.byref(d), C.byref(ev)) == _capi.MGN_E_ARG, bad
    still_works()
    # the training entry points answer solver 2 as before: a value they do not know
    d.solver, d.out = 2, None
    g, lv = np.zeros(eng.param_count, F32), C.c_float()
    assert eng.lib.mgn_solver_grad(eng.h, C.byref(d), _capi.f32(gt), None, None, 0.0, _capi.f32(g), g.size, C.byref(lv)) == _capi.MGN_E_ARG
    assert "solver must be 0" in eng.lib.mgn_last_error(eng.h).decode()
    o = _capi.MgnSolverGradOpts()
    assert eng.lib.mgn_solver_grad_tsit5(eng.h, C.byref(d), C.byref(o), _capi.f32(gt), None, None, 0.0, _capi.f32(g), g.size,
                                         C.byref(lv)) == _capi.MGN_E_ARG
    del keep
    still_works()
