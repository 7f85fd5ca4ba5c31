"""Solver-based training without a GPU: the float64 reference driver of mgn_solver_grad (tests/solver_adjoint_ref.py) against
central differences on a linear ODE, the MultipleShooting window formula, and Engine.solver_grad's argument checks on a host-only
handle."""
import numpy as np
import pytest

import solver_adjoint_ref as sar
from mgn_amd import MGN_DEVICE_NONE, Engine, MgnError, synth
from mgn_amd import _capi
from mgn_amd import reference_api as ra


def linear_problem(seed=0, N=5, O=2):
    """f(x) = A x on the flattened state; p = A (its entries are the parameters)."""
    rng = np.random.default_rng(seed)
    A = 0.5 * rng.standard_normal((N * O, N * O))
    x0 = rng.standard_normal((N, O))
    return A, x0


def linear_fns(A, N, O):
    def rhs(x):
        return (A @ np.asarray(x, np.float64).ravel()).reshape(N, O)

    def vjp(x, lam):
        lam = np.asarray(lam, np.float64).ravel()
        return (A.T @ lam).reshape(N, O), np.outer(lam, np.asarray(x, np.float64).ravel()).ravel()

    return rhs, vjp


@pytest.mark.parametrize("case", ["plain", "inflow", "substeps_l1"])
def test_reference_driver_matches_central_differences(case):
    N, O = 5, 2
    A, x0 = linear_problem(1, N, O)
    rng = np.random.default_rng(2)
    kw = dict(t0=0.0, t1=0.06, dt=0.01, saves_dt=0.01, n_saves=7)
    if case == "substeps_l1":
        kw.update(dt=0.005, cont_target=rng.standard_normal((N, O)), cont_weight=0.3)
    if case == "inflow":
        kw.update(inflow_mask=np.array([1, 0, 0, 1, 0], np.uint8), inflow_data=rng.standard_normal((8, N, O)))
    gt = rng.standard_normal((kw["n_saves"], N, O))
    vm = np.array([1, 1, 0, 1, 1], np.float64)
    ls = np.array([2.0, 0.5])
    rhs, vjp = linear_fns(A, N, O)
    gs, loss, pred, xin = sar.euler_adjoint(rhs, vjp, x0, gt, val_mask=vm, loss_scale=ls, **kw)
    assert gs.shape == (A.size,) and np.isfinite(loss)
    if case == "inflow":    # the state is not overwritten: the inflow rows of the saves are not the frames'
        assert not np.allclose(pred[1][0], kw["inflow_data"][0][0])
        assert np.array_equal(xin[0][0], kw["inflow_data"][0][0])

    def loss_at(Ap):
        r, v = linear_fns(Ap, N, O)
        return sar.euler_adjoint(r, v, x0, gt, val_mask=vm, loss_scale=ls, **kw)[1]

    eps = 1e-6
    d = rng.standard_normal(A.shape)
    fd = (loss_at(A + eps * d) - loss_at(A - eps * d)) / (2 * eps)
    assert abs(fd - float(gs @ d.ravel())) <= 1e-6 * max(1.0, abs(fd)), (fd, float(gs @ d.ravel()))
    # and every entry of a few rows: the gradient is the discrete adjoint, exactly
    for (i, j) in [(0, 0), (3, 7), (9, 2)]:
        e = np.zeros_like(A)
        e[i, j] = 1.0
        fd = (loss_at(A + eps * e) - loss_at(A - eps * e)) / (2 * eps)
        assert abs(fd - gs[i * A.shape[1] + j]) <= 1e-6 * max(1.0, abs(fd))


def test_reference_driver_save_steps_and_frames():
    ts, steps, sdt, tt = sar.time_grid(0.0, 0.1, 0.005, 0.02, 6)
    assert len(ts) == 21 and steps == [0, 4, 8, 12, 16, 20]
    assert [sar.frame_of(t, sdt, tt, 6) for t in ts[:5]] == [0, 0, 0, 0, 1]
    with pytest.raises(ValueError):
        sar.time_grid(0.0, 0.05, 0.01, 0.02, 4)          # the fourth save (t = 0.06) lies beyond t1


@pytest.mark.parametrize("T,isz,expect", [
    (10, 4, [(0, 3), (3, 6), (6, 9)]),
    (11, 4, [(0, 3), (3, 6), (6, 9), (9, 10)]),          # a short last window
    (5, 2, [(0, 1), (1, 2), (2, 3), (3, 4)]),
    (6, 10, [(0, 5)]),
    (600, 100, [(i, min(599, i + 99)) for i in range(0, 599, 99)]),
])
def test_multiple_shooting_windows(T, isz, expect):
    got = ra.multiple_shooting_ranges(T, isz)
    assert got == expect
    # the reference's formula written in Julia's 1-based terms: [i:min(T, i + isz - 1) for i in 1:(isz - 1):(T - 1)]
    jl = []
    i = 1
    while i <= T - 1:
        jl.append((i, min(T, i + isz - 1)))
        i += isz - 1
    assert [(a + 1, b + 1) for a, b in got] == jl
    assert got[0][0] == 0 and got[-1][1] == T - 1
    assert all(got[j][1] == got[j + 1][0] for j in range(len(got) - 1))


def test_multiple_shooting_rejects_interval_size_one():
    with pytest.raises(ValueError):
        ra.multiple_shooting_ranges(10, 1)


def test_solver_grad_prototype_is_bound(lib_built):
    lib = _capi.load()
    assert "mgn_solver_grad" in _capi.PROTOTYPES and hasattr(lib, "mgn_solver_grad")


def test_solver_grad_argument_checks_host_only(lib_built):
    pos, cells = synth.grid_mesh(4, 3, 1)
    s, r = synth.cells_to_edges(cells)
    N, E = pos.shape[0], s.size
    e = Engine(9, 3, 2, L=32, mps=1, device=MGN_DEVICE_NONE)
    e.set_graph(s, r, N)
    x0 = np.zeros((N, 2), np.float32)
    oh = np.zeros((N, 7), np.float32)
    ef = np.zeros((E, 3), np.float32)
    gt = np.zeros((3, N, 2), np.float32)
    args = (x0, oh, ef, gt, 0.0, 0.02, 0.01, 0.01, 3)
    with pytest.raises(ValueError):                        # gt of the wrong shape
        e.solver_grad(x0, oh, ef, gt[:2], 0.0, 0.02, 0.01, 0.01, 3)
    with pytest.raises(ValueError):                        # x0 of the wrong shape
        e.solver_grad(x0[:-1], oh, ef, gt, 0.0, 0.02, 0.01, 0.01, 3)
    with pytest.raises(ValueError):
        e.solver_grad(*args, loss_scale=np.ones(3))
    with pytest.raises(ValueError):
        e.solver_grad(*args, cont_target=np.zeros((N, 3)), cont_weight=1.0)
    with pytest.raises(ValueError):                        # mask without frames
        e.solver_grad(*args, inflow_mask=np.zeros(N, np.uint8))
    with pytest.raises(ValueError):
        e.solver_grad(*args, inflow_rule="nearest")
    with pytest.raises(ValueError):
        e.solver_grad(x0, oh, ef, gt[:0], 0.0, 0.02, 0.01, 0.01, 0)
    with pytest.raises(ValueError):
        e.solver_grad(*args, out=np.zeros(e.param_count - 1, np.float32))
    with pytest.raises(MgnError) as ei:                    # well-formed: the C ABI answers, and a host-only handle has no compute path
        e.solver_grad(*args)
    assert ei.value.code == _capi.MGN_E_HIP
    e.close()
