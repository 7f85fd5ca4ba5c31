"""Tsit5 window gradients with interpolated saves (MGN_TSIT5_DENSE_SAVES), the part that needs no GPU: the dense-output weights behind
mgn_tsit5_interp_weights against the tableau and the order conditions, the float64 reference driver (tests/tsit5_dense_ref.py) against
central differences on a small smooth right-hand side, the save plan in both time types, the step-mode flags through the ABI on a
host-only handle, and the Python entry points.  The device side is tests/test_gpu_solver_train_tsit5_dense.py."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import mgn_amd
import tsit5_dense_ref as tdr
from mgn_amd import MGN_DEVICE_NONE, Engine, GroupEngine, _capi
from mgn_amd import reference_api as ra


def weights(lib, theta):
    b = np.full(7, np.nan)
    rc = lib.mgn_tsit5_interp_weights(float(theta), b.ctypes.data_as(C.POINTER(C.c_double)))
    return rc, b


def test_interp_weights_match_the_tableau_and_the_order_conditions(lib_built):
    lib = mgn_amd.load()
    rc, b = weights(lib, 1.0)
    assert rc == _capi.MGN_OK
    assert np.abs(b[:6] - np.asarray(ra.TSIT5_A[6])).max() <= 1e-14 and abs(b[6]) <= 1e-14          # b(1) is the method's b; b_7(1) = 0
    A = np.zeros((7, 7))
    A[:, :6] = np.asarray(ra.TSIT5_A)
    c = np.asarray(ra.TSIT5_C)
    for theta in (0.0, 0.2, 0.4, 0.77, 1.0):
        rc, b = weights(lib, theta)
        assert rc == _capi.MGN_OK
        assert abs(b.sum() - theta) <= 1e-13
        assert abs(b @ c - theta ** 2 / 2) <= 1e-13
        assert abs(b @ c ** 2 - theta ** 3 / 3) <= 1e-13
        assert abs(b @ (A @ c) - theta ** 3 / 6) <= 1e-13
        assert np.abs(b - tdr.interp_weights(theta)).max() <= 1e-14                                 # the tests' own copy of the constants
    for theta in (-1e-9, 1.0 + 1e-9, float("nan"), float("inf")):
        assert weights(lib, theta)[0] == _capi.MGN_E_ARG
    assert lib.mgn_tsit5_interp_weights(0.5, None) == _capi.MGN_E_ARG


def tanh_fns(W):
    def rhs(x):
        return np.tanh(np.asarray(x, np.float64) @ W)

    def vjp(x, lam):
        x = np.asarray(x, np.float64)
        ub = np.asarray(lam, np.float64) * (1.0 - np.tanh(x @ W) ** 2)
        return ub @ W.T, (x.T @ ub).ravel()

    return rhs, vjp


def test_reference_adjoint_matches_central_differences():
    """Steps [0, 0.025, 0.05], saves every 0.01: saves 1, 2 inside the first step, 3, 4 inside the last (the FSAL term into step 1's first
    stage, and the extra VJP at z_{K,1}), save 5 on the end.  Inflow rows, so the stage inputs are copies and the cotangents are masked."""
    N, O = 6, 2
    rng = np.random.default_rng(3)
    W = 0.9 * rng.standard_normal((O, O))
    x0 = rng.standard_normal((N, O))
    step_t, step_h, t_end = [0.0, 0.025], [0.025, 0.025], 0.05
    plan = tdr.dense_plan(step_t, step_h, t_end, 0.0, 0.01, 6, np.float64)
    assert [(i, hit) for i, _, hit in plan] == [(0, True), (0, False), (0, False), (1, False), (1, False), (2, True)]
    assert np.allclose([th for _, th, hit in plan if not hit], [0.4, 0.8, 0.2, 0.6], atol=1e-12)
    gt = rng.standard_normal((6, N, O))
    frames = rng.standard_normal((6, N, O))
    kw = dict(val_mask=np.array([1, 1, 0, 1, 1, 1.0]), inflow_mask=np.array([1, 0, 0, 1, 0, 0], np.uint8), inflow_data=frames,
              loss_scale=np.array([2.0, 0.5]), cont_target=rng.standard_normal((N, O)), cont_weight=0.3, time_type=np.float64)

    def run(Wq, xq):
        r, v = tanh_fns(Wq)
        return tdr.tsit5_dense_adjoint(r, v, xq, gt, step_t, step_h, t_end, plan, 0.01, **kw)

    gs, loss, pred, zs, xbar0 = run(W, x0)
    assert pred.shape == (6, N, O) and np.array_equal(pred[0], x0) and np.isfinite(loss)
    eps = 1e-6
    for i in range(W.size):
        e = np.zeros(W.size)
        e[i] = eps
        fd = (run(W + e.reshape(O, O), x0)[1] - run(W - e.reshape(O, O), x0)[1]) / (2 * eps)
        assert abs(fd - gs[i]) <= 1e-6 * max(1.0, abs(fd)), (i, fd, gs[i])
    for i in range(x0.size):
        e = np.zeros(x0.size)
        e[i] = eps
        fd = (run(W, x0 + e.reshape(N, O))[1] - run(W, x0 - e.reshape(N, O))[1]) / (2 * eps)
        assert abs(fd - xbar0.ravel()[i]) <= 1e-6 * max(1.0, abs(fd)), (i, fd, xbar0.ravel()[i])
    # without interpolated saves the driver is its twin
    import tsit5_adjoint_ref as tar
    r, v = tanh_fns(W)
    plan_h = [(0, None, True), (1, None, True), (2, None, True)]
    a = tdr.tsit5_dense_adjoint(r, v, x0, gt[:3], step_t, step_h, t_end, plan_h, 0.025, **kw)
    b = tar.tsit5_adjoint(r, v, x0, gt[:3], step_t, step_h, [0, 1, 2], 0.025, **kw)
    assert abs(a[1] - b[1]) <= 1e-14 * abs(b[1]) and np.abs(a[0] - b[0]).max() <= 1e-13 * np.abs(b[0]).max()


@pytest.mark.parametrize("time_type", [np.float32, np.float64])
def test_save_plan(time_type):
    tt = (lambda v: float(np.float32(v))) if time_type == np.float32 else float
    # fixed steps of 0.015 to t1 = 0.04: the last step is cut to 0.01; saves 1 and 2 are interpolated, save 3 sits on the second step's
    # end (2 * 0.015 is 3 * 0.01 in both types), save 4 on t1
    st, sh, t_end = tdr.fixed_dense_steps(0.0, tt(0.04), 0.015, 0.01, time_type)
    assert len(sh) == 3 and sh[0] == sh[1] == tt(0.015) and abs(sh[2] - 0.01) < 1e-7 and t_end == tt(0.04)
    plan = tdr.dense_plan(st, sh, t_end, 0.0, 0.01, 5, time_type)
    assert [(i, hit) for i, _, hit in plan] == [(0, True), (0, False), (1, False), (2, True), (3, True)]
    assert np.allclose([th for _, th, hit in plan if not hit], [2 / 3, 1 / 3], atol=1e-6)
    assert all(0.0 <= th <= 1.0 for _, th, hit in plan if not hit)
    # a save that hits a step end is that state; steps that straddle saves interpolate them
    st, sh, t_end = [0.0, tt(0.02), tt(0.035)], [tt(0.02), tt(0.035) - tt(0.02), tt(0.05) - tt(0.035)], tt(0.05)
    t_end = tt(tt(0.0) + 5 * tt(0.01))                                   # the save grid's own end (an ulp below float32(0.05))
    plan = tdr.dense_plan(st, sh, t_end, 0.0, 0.01, 6, time_type)
    assert [(i, hit) for i, _, hit in plan] == [(0, True), (0, False), (1, True), (1, False), (2, False), (3, True)]
    # a save an ulp beyond t1 is the final state
    t1 = float(np.nextafter(time_type(t_end), time_type(0.0)))
    plan = tdr.dense_plan(st, sh, t1, 0.0, 0.01, 6, time_type)
    assert plan[5] == (3, None, True) and not plan[4][2]
    # the fixed grid with dt = saves_dt: every save sits on a state
    st, sh, t_end = tdr.fixed_dense_steps(0.0, tt(0.04), 0.01, 0.01, time_type)
    assert [p[0] for p in tdr.dense_plan(st, sh, t_end, 0.0, 0.01, 5, time_type)] == [0, 1, 2, 3, 4]
    assert all(p[2] for p in tdr.dense_plan(st, sh, t_end, 0.0, 0.01, 5, time_type))


def test_step_mode_flags_through_the_abi_on_a_host_build(lib_built):
    assert (_capi.MGN_TSIT5_ADAPTIVE, _capi.MGN_TSIT5_DENSE_SAVES) == (1, 2)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mgn_hip.h")).read()
    assert "#define MGN_TSIT5_ADAPTIVE 1" in hdr and "#define MGN_TSIT5_DENSE_SAVES 2" in hdr
    e = Engine(9, 3, 2, device=MGN_DEVICE_NONE)
    N = 4
    x0, oh, ef = np.zeros((N, 2), np.float32), np.zeros((N, 7), np.float32), np.zeros((1, 3), np.float32)
    gt = np.zeros((2, N, 2), np.float32)
    d = _capi.MgnRolloutDesc()
    d.solver, d.t0, d.t1, d.dt, d.saves_dt, d.n_saves, d.abstol, d.reltol = 1, 0.0, 0.01, 0.01, 0.01, 2, 1e-6, 1e-3
    d.x0, d.node_type_onehot, d.ef_raw = _capi.f32(x0), _capi.f32(oh), _capi.f32(ef)
    gs, loss = np.zeros(e.param_count, np.float32), C.c_float()

    def call(handle_call, h, mode):
        o = _capi.MgnSolverGradOpts()
        o.adaptive = mode
        return handle_call(h, C.byref(d), C.byref(o), _capi.f32(gt), None, None, 0.0, _capi.f32(gs), gs.size, C.byref(loss))

    for mode in (4, 8, 5, -1):                   # any bit but the two flags: a bad argument, whatever the handle can compute
        assert call(e.lib.mgn_solver_grad_tsit5, e.h, mode) == _capi.MGN_E_ARG, mode
    for mode in (0, 1, 2, 3):                    # the four modes reach the handle's own answer: no compute path here
        assert call(e.lib.mgn_solver_grad_tsit5, e.h, mode) == _capi.MGN_E_HIP, mode
    e.close()
    with GroupEngine(9, 3, 2, devices=[MGN_DEVICE_NONE] * 2) as g:
        for mode in (4, 8):
            assert call(g.lib.mgn_group_solver_grad_tsit5, g.g, mode) == _capi.MGN_E_ARG, mode


class _Recorder:
    """Engine.solver_grad_tsit5's signature, recording the keywords of every call"""

    def __init__(self):
        self.calls = []

    def solver_grad_tsit5(self, x0, node_type_onehot, ef_raw, gt, t0, t1, saves_dt, n_saves, **kw):
        self.calls.append(kw)
        return np.ones(3), 1.0, {}


def test_python_entry_points():
    for cls in (Engine, GroupEngine):
        p = inspect.signature(cls.solver_grad_tsit5).parameters["dense_saves"]
        assert p.default is False
    assert inspect.signature(ra.train_step_multiple_shooting).parameters["interpolate_saves"].default is False
    gt = np.zeros((7, 4, 2), np.float32)
    rec = _Recorder()
    ra.train_step_multiple_shooting(rec, gt, None, None, 0.0, 0.01, 0.06, 3, 100, solver="Tsit5")
    assert len(rec.calls) == 3 and all("dense_saves" not in kw for kw in rec.calls)            # the default: today's call
    rec = _Recorder()
    gs, loss = ra.train_step_multiple_shooting(rec, gt, None, None, 0.0, 0.01, 0.06, 3, 100, solver="Tsit5", interpolate_saves=True)
    assert len(rec.calls) == 3 and all(kw["dense_saves"] is True for kw in rec.calls) and loss == 3.0
    with pytest.raises(ValueError):
        ra.train_step_multiple_shooting(rec, gt, None, None, 0.0, 0.01, 0.06, 3, 100, solver="Tsit5", adaptive=False, batched=True,
                                        interpolate_saves=True)
    with pytest.raises(ValueError):
        ra.train_step_multiple_shooting(rec, gt, None, None, 0.0, 0.01, 0.06, 3, 100, solver="Euler", interpolate_saves=True)
