"""Solver-based training with Tsit5 without a GPU: the float64 reference driver of mgn_solver_grad_tsit5 (tests/tsit5_adjoint_ref.py)
against central differences on a small nonlinear ODE over a ring graph, reference_api.solver_training_tsit5 against the driver, and the
MgnSolverGradOpts mirrors (ctypes, Julia) and the Julia call of mgn_solver_grad_tsit5 against the header."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import test_julia_shim as js
import tsit5_adjoint_ref as tar
from mgn_amd import _capi
from mgn_amd import reference_api as ra


def ring_fns(p, N, O):
    """f(x)_n = tanh(W x_n + M (x_{n-1} + x_{n+1}) + b) on a ring of N nodes; p = [W, M, b] flattened."""
    W, M, b = p[:O * O].reshape(O, O), p[O * O:2 * O * O].reshape(O, O), p[2 * O * O:]

    def nb(x):
        return np.roll(x, 1, axis=0) + np.roll(x, -1, axis=0)

    def rhs(x):
        x = np.asarray(x, np.float64)
        return np.tanh(x @ W.T + nb(x) @ M.T + b)

    def vjp(x, lam):
        x = np.asarray(x, np.float64)
        y = np.tanh(x @ W.T + nb(x) @ M.T + b)
        ub = np.asarray(lam, np.float64) * (1.0 - y * y)
        xbar = ub @ W + nb(ub) @ M
        return xbar, np.concatenate([(ub.T @ x).ravel(), (ub.T @ nb(x)).ravel(), ub.sum(0)])

    return rhs, vjp


def ring_problem(seed=0, N=6, O=2):
    rng = np.random.default_rng(seed)
    p = np.concatenate([0.8 * rng.standard_normal(2 * O * O), 0.3 * rng.standard_normal(O)])
    return p, rng.standard_normal((N, O)), rng


@pytest.mark.parametrize("time_type", [np.float32, np.float64])
@pytest.mark.parametrize("mode", ["fixed", "varying"])
def test_driver_matches_central_differences(mode, time_type):
    N, O = 6, 2
    p, x0, rng = ring_problem(1, N, O)
    if mode == "fixed":          # dt = 0.03 across saves of 0.02: inflow frames change inside steps
        step_t, step_h, save_step, _ = tar.fixed_steps(0.0, 0.06, 0.03, 0.02, 4, time_type)
        assert len(step_h) == 2
    else:                        # an adaptive-looking sequence, frozen
        step_h = [0.013, 0.021, 0.026]
        step_t = [0.0, 0.013, 0.034]
        tt = (lambda v: float(np.float32(v))) if time_type == np.float32 else float
        step_t = [tt(t) for t in step_t]
        save_step = [0, 2, 3, 3]
    n_saves = len(save_step)
    gt = rng.standard_normal((n_saves, N, O))
    frames = rng.standard_normal((5, N, O))
    im = np.array([1, 0, 0, 1, 0, 0], np.uint8)
    kw = dict(val_mask=np.array([1, 1, 0, 1, 1, 1.0]), inflow_mask=im, inflow_data=frames, loss_scale=np.array([2.0, 0.5]),
              cont_target=rng.standard_normal((N, O)), cont_weight=0.3, time_type=time_type)
    rhs, vjp = ring_fns(p, N, O)
    gs, loss, pred, zs = tar.tsit5_adjoint(rhs, vjp, x0, gt, step_t, step_h, save_step, 0.02, **kw)
    assert gs.shape == p.shape and np.isfinite(loss)
    # the stage inputs carry the frames' rows; some step sees two different frames among its stages
    frs = [[int(np.argmin([np.abs(z[im.astype(bool)] - f[im.astype(bool)]).max() for f in frames])) for z in zn] for zn in zs]
    assert any(len(set(f)) > 1 for f in frs), frs

    def loss_at(q):
        r, v = ring_fns(q, N, O)
        return tar.tsit5_adjoint(r, v, x0, gt, step_t, step_h, save_step, 0.02, **kw)[1]

    eps = 1e-6
    for _ in range(3):
        d = rng.standard_normal(p.shape)
        fd = (loss_at(p + eps * d) - loss_at(p - eps * d)) / (2 * eps)
        assert abs(fd - float(gs @ d)) <= 1e-6 * max(1.0, abs(fd)), (fd, float(gs @ d))
    for i in range(p.size):
        e = np.zeros_like(p)
        e[i] = 1.0
        fd = (loss_at(p + eps * e) - loss_at(p - eps * e)) / (2 * eps)
        assert abs(fd - gs[i]) <= 1e-6 * max(1.0, abs(fd)), (i, fd, gs[i])


def test_tableau_is_consistent():
    A = np.asarray(ra.TSIT5_A)
    assert A.shape == (7, 6) and abs(A[6].sum() - 1.0) < 1e-12            # b sums to one
    assert all(abs(A[i].sum() - ra.TSIT5_C[i]) < 1e-12 for i in range(1, 6))  # row sums are the nodes


def test_host_composition_matches_driver():
    N, O = 6, 2
    p, x0, rng = ring_problem(2, N, O)
    step_h = [0.011, 0.017, 0.02, 0.012]
    step_t = list(np.cumsum([0.0] + step_h[:-1]))
    save_step = [0, 1, 3, 4]
    gt = rng.standard_normal((4, N, O))
    vm, ls = np.array([1, 0, 1, 1, 1, 1.0]), np.array([1.5, 0.7])
    ct = rng.standard_normal((N, O))
    rhs, vjp = ring_fns(p, N, O)
    gs, loss, _ = ra.solver_training_tsit5(rhs, vjp, x0, gt, step_t, step_h, val_mask=vm, n_scale=ls, save_step=save_step, cont_target=ct,
                                           cont_weight=0.2)
    gs_d, loss_d, _, _ = tar.tsit5_adjoint(rhs, vjp, x0, gt, step_t, step_h, save_step, 0.02, val_mask=vm, loss_scale=ls, cont_target=ct,
                                           cont_weight=0.2, time_type=np.float64)
    # the host composition hands float32 arrays to rhs / vjp (what Engine.ode_step / ode_vjp take)
    assert abs(loss - loss_d) <= 1e-5 * abs(loss_d), (loss, loss_d)
    assert np.linalg.norm(gs - gs_d) <= 1e-5 * np.linalg.norm(gs_d)


def test_adaptive_save_mapping():
    step_t = [0.0, 0.007, 0.01, 0.018, 0.02]
    assert tar.adaptive_saves(step_t, 0.03, 0.0, 0.01, 4, np.float64) == [0, 2, 4, 5]
    st, sh, ss, t_end = tar.fixed_steps(0.0, 0.1, 0.005, 0.02, 6)
    assert len(st) == 20 and ss == [0, 4, 8, 12, 16, 20] and abs(t_end - 0.1) < 1e-7


# ---- the binding ---------------------------------------------------------------------------------------------------------------------
_CT = {C.c_int32: ("i32", 0), C.c_size_t: ("size", 0), C.POINTER(C.c_double): ("f64", 1)}


def test_ctypes_opts_mirror_matches_the_header():
    cf = js.c_struct("mgn_solver_grad_opts")
    assert [n for n, _ in _capi.MgnSolverGradOpts._fields_] == [n for n, _ in cf]
    for (n, t), (_, want) in zip(_capi.MgnSolverGradOpts._fields_, cf):
        assert _CT[t] == want, (n, t, want)


def test_julia_opts_mirror_matches_the_header():
    cf = js.c_struct("mgn_solver_grad_opts")
    jf = js.julia_struct(os.path.join(js.JULIA_DIR, "MGNHip.jl"), "MgnSolverGradOpts")
    assert [n for n, _ in jf] == [n for n, _ in cf]
    for (n, jt), (_, ct) in zip(jf, cf):
        assert js._JL[jt] == ct, (n, jt, ct)


def test_prototype_and_julia_call_match_the_header(lib_built):
    protos = js.c_prototypes()
    ret, args = protos["mgn_solver_grad_tsit5"]
    assert ret == ("i32", 0)
    assert args == [("mgn_handle", 1), ("mgn_rollout_desc", 1), ("mgn_solver_grad_opts", 1), ("f32", 1), ("f32", 1), ("f32", 1),
                    ("f32", 0), ("f32", 1), ("size", 0), ("f32", 1)]
    assert "mgn_solver_grad_tsit5" in _capi.PROTOTYPES and hasattr(_capi.load(), "mgn_solver_grad_tsit5")
    assert len(_capi.PROTOTYPES["mgn_solver_grad_tsit5"][1]) == len(args)
    # the shim binds it with @ccall (typed arguments `value::Type`): every type against the header
    text = js._strip_jl_comments(open(os.path.join(js.JULIA_DIR, "MGNHip.jl")).read())
    m = re.search(r"@ccall\s+LIB\.mgn_solver_grad_tsit5\(", text)
    assert m
    i, depth = m.end(), 1
    while depth:
        depth += {"(": 1, ")": -1}.get(text[i], 0)
        i += 1
    parts = js._split_top(text[m.end():i - 1])
    rtype = re.match(r"::(\w+)", text[i:]).group(1)
    assert js._compatible(js._JL[rtype], ret)
    assert len(parts) == len(args)
    jl = dict(js._JL, **{"Ref{MgnSolverGradOpts}": ("mgn_solver_grad_opts", 1)})
    for k, (a, c) in enumerate(zip(parts, args)):
        t = a.rsplit("::", 1)[1].strip()
        assert js._compatible(jl[t], c), (k, a, c)
