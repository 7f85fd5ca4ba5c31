"""mgn_rollout_erk / mgn_rollout_eval_erk and their group forms (Engine.rollout with "RK4", "BS3", ..., or an ErkTableau): explicit
Runge-Kutta methods given as a Butcher tableau, through the time loops of mgn_rollout.

References: MGN_SOLVER_EULER, MGN_SOLVER_TSIT5_FIXED and MGN_SOLVER_TSIT5 bit for bit for the Euler and Tsit5 tableaux (the same loops,
handed the same coefficients); the training form (Engine.solver_grad_tsit5(adaptive=False)) bit for bit where there is no inflow mask;
a host replay of the fixed-step loop in NumPy float32 on the engine's own right-hand side (tests/erk_ref.py), with a perturbed tableau
to show that the comparison can tell two methods apart; the same tableau at saves_dt / 8 for the adaptive runs; the coherent numbering;
one partition.  Fixtures: the 150-point cylinder of tests/test_gpu_solver_train.py (L = 64, mps = 2, K = 4 save periods), 151 points
where the element count must not be a multiple of four, the 1320-node grid of tests/group_solver_case.py for the partitions.  Run on
the MI355X with `-m gpu`; every test prints its figures before it asserts.

Measured on the MI355X, dt = saves_dt = 0.01, four steps, with the inflow mask, rel_max against the host replay (bound 4 x noise) and
against the replay with two coefficients swapped (must exceed 40 x noise):
  150 points: noise 5.24e-7 (bound 2.1e-6, power bound 2.1e-5); Heun 1.27e-7 / 6.3e-2, Midpoint 1.27e-7 / 4.3e-3, Ralston 1.27e-7 /
              2.8e-3, RK4 6.3e-8 / 1.03e-4, BS3 1.27e-7 / 4.7e-4, DP5 1.27e-7 / 1.5e-4
  151 points: noise 2.88e-7 (bound 1.2e-6, power bound 1.2e-5); Heun 1.15e-7 / 6.0e-2, Midpoint 1.15e-7 / 7.0e-3, Ralston 1.15e-7 /
              4.3e-3, RK4 1.15e-7 / 1.14e-4, BS3 1.73e-7 / 7.4e-4, DP5 1.15e-7 / 2.5e-4
  so dt = 0.01 tells every pair apart and B.4 runs there.
Adaptive (first step 0.004) against the same tableau at saves_dt / 8, relative L2: BS3 4.2e-6 at reltol 1e-3 (14 steps, bound 1.4e-2),
  2.2e-6 at 1e-5 (22 steps, 1 rejected, bound 2.5e-4); DP5 1.2e-5 at 1e-3 (6 steps, bound 6.0e-3), 5.1e-6 at 1e-5 (9 steps, bound
  1.0e-4).  With the Hairer-Wanner start: BS3 17 / 25 steps, DP5 4 / 4 (one step per save period), one more right-hand side each.
Groups of 2 / 3 ranks against one partition, rel_max: RK4 1.2e-7 / 1.2e-7, BS3 2.4e-7 / 1.8e-7 (tolerance 1e-5; equal counters)
Renumbered (400 points) against the coherent numbering, relative L2: RK4 3.5e-8, BS3 9.9e-8 (tolerance 1e-3)
bf16 handle (L = 128), RK4, against the fp32 replay: relative L2 1.6e-4 (band 3e-2)"""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch   # noqa: F401  (before the engine's first HIP call)

import erk_ref
import solver_adjoint_ref as sar
from group_solver_case import case, setup
from mgn_amd import MgnError, _capi, erk_tableau
from test_gpu_group_solver_train import TOL_FWD, assert_partitioned, check_reductions, group, same_bits
from test_gpu_solver_train import problem
from util import TOL_ROLLOUT, engine_for, rel_max, renumbered

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SDT = 0.01
K = 4
TOL_BF16 = 3e-2      # relative L2, DESIGN.md section 2
OTHERS = ("Heun", "Midpoint", "Ralston", "RK4", "BS3", "DP5")
STAGES = dict(Euler=1, Heun=2, Midpoint=2, Ralston=2, RK4=4, BS3=4, DP5=7, Tsit5=7)
FSAL = ("BS3", "DP5", "Tsit5")


@functools.lru_cache(maxsize=None)
def prob(**kw):
    """this module's own test_gpu_solver_train.problem, made once per shape (its engine keeps no state between calls)"""
    return problem(K=K, **kw)


@functools.lru_cache(maxsize=None)
def grid_engine():
    """this module's own unpartitioned Engine of group_solver_case.case()"""
    pr = case()
    e = engine_for(pr["cfg"])
    setup(e, pr)
    return e


def t_at(i, time_type=F32):
    tt = np.dtype(time_type).type
    return float(tt(i * float(tt(SDT))))


def inflow_of(P, n_frames, seed=21):
    im = ((P["node_type"] == 4) | (P["node_type"] == 1)).astype(np.uint8)
    assert im.any() and not im.all()
    frames = (P["gt"][0][None] * (1.0 + 0.2 * np.random.default_rng(seed).standard_normal((n_frames, P["N"], 2)))).astype(F32)
    return im, frames


def roll(eng, P, solver, dt=SDT, x0=None, **kw):
    x0 = P["gt"][0] if x0 is None else x0
    tt = kw.get("time_type", F32)
    return eng.rollout(solver, x0, P["onehot"], P["ef_raw"], 0.0, t_at(K, tt), SDT, K + 1, dt=dt, val_mask=P["vm"], **kw)


def host_replay(eng, P, tab, dt=SDT, **kw):
    eng.set_static(P["onehot"], P["ef_raw"], P["vm"])
    tt = kw.get("time_type", F32)
    return erk_ref.replay(lambda x: eng.ode_step(np.ascontiguousarray(x, F32)), tab, P["gt"][0], 0.0, t_at(K, tt), dt, SDT, K + 1, **kw)


def n_rhs_of(name, st):
    s, trials = STAGES[name], st["n_accept"] + st["n_reject"]
    return 1 + (s - 1) * trials if name in FSAL else st["n_accept"] + (s - 1) * trials


# ---- B.1: the Euler tableau is MGN_SOLVER_EULER ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor", [1.0, 0.5])
@pytest.mark.parametrize("masked", [False, True])
def test_euler_tableau_returns_the_bits_of_solver_euler(factor, masked):
    P = prob()
    eng = P["eng"]
    im, frames = inflow_of(P, K + 2)
    kw = dict(inflow_mask=im, inflow_data=frames) if masked else dict()
    ref, st_ref = roll(eng, P, "Euler", factor * SDT, **kw)
    for adaptive in (False, True):                     # no embedded pair: `adaptive` is ignored, as "Euler" ignores it
        sol, st = roll(eng, P, erk_tableau("Euler"), factor * SDT, adaptive=adaptive, **kw)
        assert same_bits(sol, ref) and st == st_ref == dict(n_accept=int(K / factor), n_reject=0, n_rhs=int(K / factor))
    assert same_bits(sol[0], P["gt"][0]) and np.isfinite(sol).all() and not same_bits(sol[1], sol[0])


# ---- B.2: the Tsit5 tableau with fixed steps is MGN_SOLVER_TSIT5_FIXED ------------------------------------------------------------------
@pytest.mark.parametrize("n_points", [150, 151])
@pytest.mark.parametrize("time_type", [F32, F64], ids=["float32", "float64"])
def test_tsit5_tableau_fixed_returns_the_bits_of_solver_tsit5_fixed(time_type, n_points):
    """dt = saves_dt: the accumulated step times equal the save times exactly over these four steps in both time types, so the dense-save
    loop of MGN_SOLVER_TSIT5_FIXED and the fixed grid of mgn_rollout_erk take the same steps and every save sits on a step end"""
    P = prob(n_points=n_points)
    eng = P["eng"]
    im, frames = inflow_of(P, K + 2)
    kw = dict(inflow_mask=im, inflow_data=frames, time_type=time_type)
    ref, st_ref = roll(eng, P, "Tsit5", adaptive=False, **kw)
    sol, st = roll(eng, P, erk_tableau("Tsit5"), adaptive=False, **kw)
    assert st == st_ref == dict(n_accept=K, n_reject=0, n_rhs=1 + 6 * K)
    assert same_bits(sol, ref) and same_bits(sol[0], P["gt"][0]) and np.isfinite(sol).all()
    m = im.astype(bool)
    ts, _, sdt, tt = sar.time_grid(0.0, t_at(K, time_type), SDT, SDT, K + 1, time_type)
    for s in range(1, K + 1):                         # FSAL: a saved x_{n+1} carries the rows of frame(t_{n+1}), by the reference's rule
        assert same_bits(sol[s][m], frames[sar.frame_of(ts[s], sdt, tt, len(frames))][m]), s


@pytest.mark.parametrize("time_type", [F32, F64], ids=["float32", "float64"])
def test_tsit5_tableau_at_half_steps_returns_the_bits_of_the_training_form(time_type):
    """dt = saves_dt / 2, no inflow mask: the fixed-step training form shares the grid and the launches"""
    P = prob()
    eng, gt = P["eng"], P["gt"]
    dt, t1 = 0.5 * SDT, t_at(K, time_type)
    sol, st = roll(eng, P, erk_tableau("Tsit5"), dt, adaptive=False, time_type=time_type)
    _, _, tr = eng.solver_grad_tsit5(gt[0], P["onehot"], P["ef_raw"], gt, 0.0, t1, SDT, K + 1, dt=dt, adaptive=False, dense_saves=False,
                                     val_mask=P["vm"], time_type=time_type, want_pred=True)
    assert tr["n_steps"] == 2 * K and st == dict(n_accept=2 * K, n_reject=0, n_rhs=1 + 12 * K)
    assert same_bits(sol, tr["pred"])


# ---- B.3: the Tsit5 tableau, adaptive, is MGN_SOLVER_TSIT5 ------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [0.0, 0.004])
@pytest.mark.parametrize("reltol", [1e-3, 1e-5])
def test_tsit5_tableau_adaptive_returns_the_bits_and_counters_of_solver_tsit5(reltol, dt):
    P = prob()
    eng = P["eng"]
    im, frames = inflow_of(P, K + 2)
    kw = dict(inflow_mask=im, inflow_data=frames, reltol=reltol)
    ref, st_ref = roll(eng, P, "Tsit5", dt, **kw)
    sol, st = roll(eng, P, erk_tableau("Tsit5"), dt, **kw)
    print("adaptive Tsit5, reltol %g, dt %g: %s" % (reltol, dt, st))
    # (dt = 0: the Hairer-Wanner start evaluates one more right-hand side, as it always has)
    assert st == st_ref and st["n_accept"] >= K and st["n_rhs"] == (dt == 0.0) + 1 + 6 * (st["n_accept"] + st["n_reject"])
    assert same_bits(sol, ref)


# ---- B.4: every other named tableau, fixed steps, against the host replay ------------------------------------------------------------
class Perturbed(types.SimpleNamespace):
    pass


def perturbed(tab):
    """the tableau with two non-equal coefficients swapped: b[0] and b[1] for two stages (Heun's are equal: a21 and b[0] there), the
    first two non-equal entries of the last row of A otherwise"""
    A, b = tab.A, tab.b
    s = tab.stages
    if s == 2 and b[0] != b[1]:
        b[[0, 1]] = b[[1, 0]]
    elif s == 2:
        A[1, 0], b[0] = b[0], A[1, 0]
    else:
        row = A[s - 1, :s - 1]
        i, j = next((i, j) for i in range(s - 1) for j in range(i + 1, s - 1) if row[i] != row[j])
        row[[i, j]] = row[[j, i]]
    return Perturbed(A=A, b=b, c=tab.c, stages=s, fsal=tab.fsal)


@pytest.mark.parametrize("n_points", [150, 151])
def test_named_tableaux_fixed_steps_against_the_host_replay(n_points):
    """dt = saves_dt = 0.01, four steps, with the inflow mask.  noise: rel_max of the Tsit5-tableau run (pinned bit for bit by B.2)
    against the same replay function; every tableau is held to 4 x noise (the margin of tests/test_gpu_rollout_tsit5_fixed.py: a stage
    more or less changes the rounding, not the scale), and a replay with two coefficients swapped must differ from the native result
    by more than 10 x 4 x noise: the comparison tells methods apart."""
    P = prob(n_points=n_points)
    eng = P["eng"]
    im, frames = inflow_of(P, K + 2)
    kw = dict(inflow_mask=im, inflow_data=frames)
    t5 = erk_tableau("Tsit5")
    sol5, _ = roll(eng, P, t5, adaptive=False, **kw)
    noise = rel_max(sol5, host_replay(eng, P, t5, **kw)[0])
    print("%d points: noise (Tsit5 tableau against the replay) %.3e" % (n_points, noise))
    figures = {}
    for name in OTHERS:
        tab = erk_tableau(name)
        sol, st = roll(eng, P, tab, adaptive=False, **kw)
        ref, rst = host_replay(eng, P, tab, **kw)
        wrong, _ = host_replay(eng, P, perturbed(tab), **kw)
        figures[name] = (rel_max(sol, ref), rel_max(sol, wrong), st, rst)
        print("%d points: %-8s rel_max %.3e   against the perturbed replay %.3e   %s" % (n_points, name, figures[name][0], figures[name][1], st))
        assert same_bits(sol[0], P["gt"][0]) and np.isfinite(sol).all()
    assert 0.0 < noise <= 1e-5
    for name, (err, power, st, rst) in figures.items():
        assert st == rst == dict(n_accept=K, n_reject=0, n_rhs=n_rhs_of(name, dict(n_accept=K, n_reject=0))), name
        assert err <= 4.0 * noise, (name, err, noise)
        assert power > 10.0 * 4.0 * noise, (name, power, noise)
    assert [figures[n][2]["n_rhs"] for n in OTHERS] == [2 * K, 2 * K, 2 * K, 4 * K, 1 + 3 * K, 1 + 6 * K]


# ---- B.5: adaptive BS3 and DP5 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reltol", [1e-3, 1e-5])
@pytest.mark.parametrize("name", ["BS3", "DP5"])
def test_adaptive_embedded_pairs_against_fine_fixed_steps(name, reltol):
    """reference: the same tableau at fixed dt = saves_dt / 8 (the fixed-step loop, held to the replay by B.4).  Bound on the relative
    L2 distance: n_accept (reltol + abstol / rms(x)), the sum of the controller's per-step bounds in its own RMS norm (four save
    periods; no growth factor is claimed).  First step 0.004, so that n_rhs is the FSAL formula; with dt = 0 the Hairer-Wanner start (its
    exponent 1 / p) costs one more right-hand side."""
    P = prob()
    eng = P["eng"]
    abstol = 1e-6
    sol, st = roll(eng, P, name, 0.004, reltol=reltol, abstol=abstol)
    auto, st0 = roll(eng, P, name, 0.0, reltol=reltol, abstol=abstol)
    print("adaptive %s, reltol %g, Hairer-Wanner start: %s" % (name, reltol, st0))
    assert np.isfinite(auto).all() and st0["n_rhs"] == 1 + n_rhs_of(name, st0)
    ref, _ = roll(eng, P, name, SDT / 8, adaptive=False)
    err = float(np.linalg.norm(sol.astype(F64) - ref) / np.linalg.norm(ref.astype(F64)))
    rms = float(np.sqrt(np.mean(ref.astype(F64) ** 2)))
    bound = st["n_accept"] * (reltol + abstol / rms)
    print("adaptive %s, reltol %g: %s, relative L2 against dt = saves_dt / 8: %.3e (bound %.3e)" % (name, reltol, st, err, bound))
    assert np.isfinite(sol).all() and same_bits(sol[0], P["gt"][0])
    assert st["n_accept"] >= K and st["n_rhs"] == n_rhs_of(name, st)
    assert err <= bound


# ---- B.6: rollout_eval ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver,kw", [("RK4", dict(dt=0.5 * SDT)), ("BS3", dict(dt=0.0, adaptive=True))], ids=["RK4-fixed", "BS3-adaptive"])
def test_rollout_eval_reduces_every_save_with_and_without_a_solution_buffer(solver, kw):
    P = prob()
    eng, gt = P["eng"], P["gt"]
    x0 = (gt[0] * F32(1.02)).astype(F32)
    im, _ = inflow_of(P, K + 1)
    sel = np.arange(3, 2 * P["N"], 7, dtype=np.int32)
    a = (solver, x0, P["onehot"], P["ef_raw"])
    k = dict(val_mask=P["vm"], inflow_mask=im, inflow_data=gt, inflow_rule="tolerant", **kw)
    sol, st = eng.rollout(*a, 0.0, t_at(K), SDT, K + 1, **k)
    for s_, b_ in ((None, 0), (sel + 1, 1)):
        r = eng.rollout_eval(*a, gt, 0.0, t_at(K), SDT, K + 1, sel=s_, sel_index_base=b_, want_pred=True, **k)
        assert same_bits(r["pred"], sol) and r["stats"] == st
        check_reductions(r, r["pred"], gt, s_, b_)
        q = eng.rollout_eval(*a, gt, 0.0, t_at(K), SDT, K + 1, sel=s_, sel_index_base=b_, **k)
        assert q["pred"] is None and q["stats"] == st
        assert np.float64(q["val_loss"]).tobytes() == np.float64(r["val_loss"]).tobytes()
        assert same_bits(q["mse_save"], r["mse_save"]) and same_bits(q["mse_time"], r["mse_time"])


# ---- B.7: partitions -----------------------------------------------------------------------------------------------------------------------
def group_args(pr, solver):
    return (solver, pr["gt"][0], pr["onehot"], pr["ef_raw"], 0.0, t_at(K), SDT, K + 1)


def group_kw(pr, solver):
    kw = dict(val_mask=pr["vm"], inflow_mask=pr["inflow_mask"], inflow_data=pr["frames"])
    return dict(kw, dt=0.5 * SDT) if solver == "RK4" else dict(kw, dt=0.0, adaptive=True)


@pytest.mark.parametrize("solver", ["RK4", "BS3"])
def test_group_of_one_returns_the_bits_of_the_engine(solver):
    pr, e = case(), grid_engine()
    a, kw = group_args(pr, solver), group_kw(pr, solver)
    ref, st1 = e.rollout(*a, **kw)
    q = e.rollout_eval(*a[:4], pr["gt"], *a[4:], **kw)
    with group(pr, 1) as g:
        sol, st = g.rollout(*a, **kw)
        r = g.rollout_eval(*a[:4], pr["gt"], *a[4:], **kw)
    assert same_bits(sol, ref) and st == st1
    assert np.float64(r["val_loss"]).tobytes() == np.float64(q["val_loss"]).tobytes() and r["stats"] == q["stats"] == st
    assert same_bits(r["mse_save"], q["mse_save"]) and same_bits(r["mse_time"], q["mse_time"])


@pytest.mark.parametrize("P", [2, 3])
@pytest.mark.parametrize("solver", ["RK4", "BS3"])
def test_groups_are_held_to_one_partition(solver, P):
    """RK4 with fixed steps takes no error norm: equal counters.  BS3's norm is reduced over the ranks, in another order than on one
    partition, so an accept decision may flip on a last bit: its counters are printed, not asserted across P"""
    pr, e = case(), grid_engine()
    a, kw = group_args(pr, solver), group_kw(pr, solver)
    ref, st1 = e.rollout(*a, **kw)
    with group(pr, P) as g:
        assert_partitioned(g, pr, P)
        sol, st = g.rollout(*a, **kw)
        r = g.rollout_eval(*a[:4], pr["gt"], *a[4:], want_pred=True, **kw)
        q = g.rollout_eval(*a[:4], pr["gt"], *a[4:], **kw)
    print("%s, P = %d against one partition: rel_max %.3e, counters %s against %s" % (solver, P, rel_max(sol, ref), st, st1))
    if solver == "RK4":
        assert st == st1 == dict(n_accept=2 * K, n_reject=0, n_rhs=8 * K)
    assert rel_max(sol, ref) <= TOL_FWD
    assert same_bits(r["pred"], sol) and r["stats"] == st
    check_reductions(r, r["pred"], pr["gt"])
    assert q["pred"] is None and np.float64(q["val_loss"]).tobytes() == np.float64(r["val_loss"]).tobytes()
    assert same_bits(q["mse_save"], r["mse_save"]) and same_bits(q["mse_time"], r["mse_time"])


# ---- B.8: other handles --------------------------------------------------------------------------------------------------------------------
def test_renumbered_handle_agrees_with_the_coherent_numbering():
    Pc, Ps = prob(n_points=400), prob(n_points=400, scramble=True)
    assert renumbered(Ps["eng"])
    perm = np.random.default_rng(3).permutation(Pc["N"]).astype(np.int32)     # util.scatter_labels(seed=3): perm[old] = new label
    inv = np.argsort(perm)
    assert np.array_equal(Ps["onehot"], Pc["onehot"][inv]) and np.array_equal(Ps["vm"], Pc["vm"][inv])
    im, frames = inflow_of(Pc, K + 2)
    x0 = Pc["gt"][0]
    for solver, kw in (("RK4", dict(dt=0.5 * SDT)), ("BS3", dict(dt=0.0))):
        ref, st_c = roll(Pc["eng"], Pc, solver, x0=x0, inflow_mask=im, inflow_data=frames, **kw)
        sol, st_s = roll(Ps["eng"], Ps, solver, x0=np.ascontiguousarray(x0[inv]), inflow_mask=np.ascontiguousarray(im[inv]),
                         inflow_data=np.ascontiguousarray(frames[:, inv]), **kw)
        back = sol[:, perm]
        err = float(np.linalg.norm(back.astype(F64) - ref) / np.linalg.norm(ref.astype(F64)))
        print("%s, renumbered against coherent: relative L2 %.3e, counters %s against %s" % (solver, err, st_s, st_c))
        if solver == "RK4":
            assert st_s == st_c
        assert err <= TOL_ROLLOUT
        assert same_bits(back[0], x0)


def test_bf16_handle_against_the_host_replay():
    """the bf16 handle's RK4 rollout (L = 128: the bf16 mode's one shape) against the replay on the fp32 engine's right-hand side"""
    P = prob(L=128)
    im, frames = inflow_of(P, K + 2)
    b = engine_for(P["cfg"], dtype="bf16")
    b.set_params(P["ps"])
    b.set_graph(P["s"], P["r"], P["N"])
    ns, ts, es = P["n_norm"].affine(2), P["t_norm"].affine(7), P["e_norm"].affine(3)
    b.set_norms(node=(np.concatenate([ns[0], ts[0]]), np.concatenate([ns[1], ts[1]])), edge=es, out=(P["o_norm"].std, P["o_norm"].mean))
    sol, st = roll(b, P, "RK4", 0.5 * SDT, inflow_mask=im, inflow_data=frames)
    ref, rst = host_replay(P["eng"], P, erk_tableau("RK4"), 0.5 * SDT, inflow_mask=im, inflow_data=frames)
    err = float(np.linalg.norm(sol.astype(F64) - ref) / np.linalg.norm(ref.astype(F64)))
    print("bf16 RK4: relative L2 against the fp32 replay %.3e" % err)
    assert st == rst
    assert 0.0 < err <= TOL_BF16
    b.close()


# ---- B.9: refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable():
    P = prob()
    eng, gt = P["eng"], P["gt"]
    before, st = roll(eng, P, "RK4", 0.5 * SDT)

    def still_works():
        again, st2 = roll(eng, P, "RK4", 0.5 * SDT)
        assert same_bits(again, before) and st2 == st

    def code_of(call):
        with pytest.raises(MgnError) as ei:
            call()
        return ei.value.code

    d, keep = eng._rollout_desc("Euler", gt[0], P["onehot"], P["ef_raw"], 0.0, t_at(K), SDT, K + 1, 0.5 * SDT, P["vm"], None, None, 1e-6, 1e-3,
                                "reference", F32)
    out = np.zeros((K + 1, P["N"], 2), F32)
    d.out = _capi.f32(out)
    ev = _capi.MgnRolloutEvalDesc()
    ev.gt, ev.n_gt = _capi.f32(gt), K + 1
    rk4 = erk_tableau("RK4")
    bad = rk4.tab.copy()
    bad[6 + 7 * 1 + 1] = 0.5                                                  # a diagonal entry: not explicit
    pbad = bad.ctypes.data_as(C.POINTER(C.c_double))
    assert eng.lib.mgn_rollout_erk(eng.h, C.byref(d), pbad, 0) == _capi.MGN_E_ARG
    assert eng.lib.mgn_rollout_eval_erk(eng.h, C.byref(d), C.byref(ev), pbad, 0) == _capi.MGN_E_ARG
    still_works()
    assert eng.lib.mgn_rollout_erk(eng.h, C.byref(d), rk4._ptr(), 1) == _capi.MGN_E_UNSUPPORTED      # adaptive without a pair
    assert eng.lib.mgn_rollout_eval_erk(eng.h, C.byref(d), C.byref(ev), rk4._ptr(), 1) == _capi.MGN_E_UNSUPPORTED
    assert eng.lib.mgn_rollout_erk(eng.h, C.byref(d), rk4._ptr(), 2) == _capi.MGN_E_ARG
    still_works()
    for tt in (F32, F64):
        for dt in (0.0, -0.5 * SDT):
            assert code_of(lambda: roll(eng, P, "RK4", dt, time_type=tt)) == _capi.MGN_E_ARG
            assert code_of(lambda: roll(eng, P, "BS3", dt, adaptive=False, time_type=tt)) == _capi.MGN_E_ARG
        assert code_of(lambda: roll(eng, P, "RK4", SDT / 2.5, time_type=tt)) == _capi.MGN_E_ARG      # saves_dt / dt = 2.5
        assert "MGN_SOLVER_TSIT5_FIXED" in str(pytest.raises(MgnError, roll, eng, P, "DP5", SDT / 2.5, adaptive=False, time_type=tt).value)
        assert code_of(lambda: roll(eng, P, "RK4", 2 * SDT, time_type=tt)) == _capi.MGN_E_ARG        # saves_dt / dt = 0.5
    assert code_of(lambda: roll(eng, P, "BS3", 0.0, reltol=0.0)) == _capi.MGN_E_ARG
    still_works()
    # d->solver is not read by the erk symbols, and mgn_rollout still refuses what it refused
    d.solver = 3
    assert eng.lib.mgn_rollout(eng.h, C.byref(d)) == _capi.MGN_E_ARG
    assert eng.lib.mgn_rollout_eval(eng.h, C.byref(d), C.byref(ev)) == _capi.MGN_E_ARG
    assert eng.lib.mgn_rollout_erk(eng.h, C.byref(d), rk4._ptr(), 0) == _capi.MGN_OK
    assert same_bits(out, before)
    del keep
    still_works()
