"""Solver-based training and the validation rollout on partitions, the part that needs no GPU: the group's five calls
(mgn_group_ode_vjp, mgn_group_forward_vjp, mgn_group_solver_grad, mgn_group_solver_grad_tsit5, mgn_group_rollout_eval) exist, are
declared, prototyped and bound; a host-only group refuses them as it refuses every compute call and stays usable; and the divisor rule
of the partitioned loss -- per-owner sums, folded in rank order, divided by the WHOLE mesh's count -- gives the whole-mesh loss of the
float64 references.  The device side is tests/test_gpu_group_solver_train.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mgn_amd
import solver_adjoint_ref as sar
import tsit5_adjoint_ref as tar
from group_solver_case import case, oracle_fns, rank_ordered, save_loss_terms
from mgn_amd import MGN_DEVICE_NONE, Engine, GroupEngine, MgnError, _capi
from mgn_amd import reference_api as ra

F32 = np.float32
SYMBOLS = ("mgn_group_ode_vjp", "mgn_group_forward_vjp", "mgn_group_solver_grad", "mgn_group_solver_grad_tsit5", "mgn_group_rollout_eval")
METHODS = ("ode_vjp", "forward_vjp", "solver_grad", "solver_grad_tsit5", "rollout_eval")


def test_symbols_are_exported_declared_and_bound(lib_built):
    lib = mgn_amd.load()
    raw = C.CDLL(lib_built)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "mgn_hip.h")).read()
    declared = set(re.findall(r"\bint (mgn_[a-z0-9_]+)\s*\(", hdr))
    for name in SYMBOLS:
        assert hasattr(raw, name), name
        assert name in declared, name
        assert name in _capi.PROTOTYPES, name
        # the arguments of the rank handle's call of the same name behind the handle
        assert _capi.PROTOTYPES[name] == _capi.PROTOTYPES[name.replace("mgn_group_", "mgn_")], name
        assert getattr(lib, name).argtypes == _capi.PROTOTYPES[name][1]
    assert not hasattr(raw, "mgn_group_shooting_grad")                      # out of scope: windows are looped over on the host
    for name in METHODS:                                                    # methods of the class: __getattr__ does not answer for them
        assert callable(GroupEngine.__dict__[name]) and callable(getattr(Engine, name)), name


def test_abi_version_is_unchanged(lib_built):
    assert mgn_amd.load().mgn_abi_version() == 4 == _capi.ABI_VERSION       # five new symbols; no struct or prototype changed


def _calls(g, P):
    gt, oh, ef, vm = P["gt"], P["onehot"], P["ef_raw"], P["vm"]
    N = P["N"]
    nf = np.zeros((N, P["cfg"]["Fn"]), F32)
    return (lambda: g.ode_vjp(gt[0], oh, ef, gt[1], val_mask=vm, want_dxdt=True),
            lambda: g.forward_vjp(nf, ef, gt[0], want_out=True),
            lambda: g.solver_grad(gt[0], oh, ef, gt, 0.0, 0.04, 0.01, 0.01, 5, val_mask=vm, want_pred=True),
            lambda: g.solver_grad_tsit5(gt[0], oh, ef, gt, 0.0, 0.04, 0.01, 5, dt=0.01, adaptive=False, val_mask=vm),
            lambda: g.solver_grad_tsit5(gt[0], oh, ef, gt, 0.0, 0.04, 0.01, 5, val_mask=vm),
            lambda: g.rollout_eval("Euler", gt[0], oh, ef, gt, 0.0, 0.04, 0.01, 5, dt=0.01, val_mask=vm, sel=np.arange(7, dtype=np.int32)),
            lambda: g.rollout_eval("Tsit5", gt[0], oh, ef, gt, 0.0, 0.04, 0.01, 5, want_pred=True))


@pytest.mark.parametrize("P", [1, 2])
def test_host_only_group_answers_e_hip_and_stays_usable(lib_built, P):
    pr = case()
    c = pr["cfg"]
    with GroupEngine(c["Fn"], c["Fe"], c["O"], c["L"], c["hidden_layers"], c["mps"], devices=[MGN_DEVICE_NONE] * P) as g:
        g.set_graph(pr["s"], pr["r"], pr["N"], mesh_pos=pr["pos"])
        for i, call in enumerate(_calls(g, pr)):
            with pytest.raises(MgnError) as ei:
                call()
            assert ei.value.code == _capi.MGN_E_HIP, (i, str(ei.value))
            assert "rank" in str(ei.value)
            assert sum(g.rank_engine(k).n_own for k in range(P)) == pr["N"]         # the ranks still answer
        # NULL descriptors: MGN_E_ARG, from the group itself
        d, o, ev = _capi.MgnRolloutDesc(), _capi.MgnSolverGradOpts(), _capi.MgnRolloutEvalDesc()
        gs, loss = np.zeros(g.param_count, F32), C.c_float()
        f = _capi.f32
        assert g.lib.mgn_group_solver_grad(g.g, None, f(pr["gt"]), None, None, 0.0, f(gs), gs.size, C.byref(loss)) == _capi.MGN_E_ARG
        assert g.lib.mgn_group_solver_grad_tsit5(g.g, None, C.byref(o), f(pr["gt"]), None, None, 0.0, f(gs), gs.size, C.byref(loss)) == _capi.MGN_E_ARG
        assert g.lib.mgn_group_solver_grad_tsit5(g.g, C.byref(d), None, f(pr["gt"]), None, None, 0.0, f(gs), gs.size, C.byref(loss)) == _capi.MGN_E_ARG
        assert g.lib.mgn_group_rollout_eval(g.g, None, C.byref(ev)) == _capi.MGN_E_ARG
        assert g.lib.mgn_group_rollout_eval(g.g, C.byref(d), None) == _capi.MGN_E_ARG
        assert g.lib.mgn_group_rollout_eval(g.g, C.byref(d), C.byref(ev)) == _capi.MGN_E_ARG       # gt NULL: every rank's own answer
        assert g.lib.mgn_group_ode_vjp(g.g, None, None, None, None, None, None, None, None, 0) == _capi.MGN_E_ARG
        assert g.lib.mgn_group_forward_vjp(g.g, None, None, None, None, None, None, 0) == _capi.MGN_E_ARG
        g.set_graph(pr["s"], pr["r"], pr["N"], mesh_pos=pr["pos"])                  # the group stays usable
        assert sum(g.rank_engine(k).n_own for k in range(P)) == pr["N"]
        with pytest.raises(TypeError):                                              # host arrays only
            g.solver_grad(pr["gt"][0], pr["onehot"], pr["ef_raw"], pr["gt"].tolist(), 0.0, 0.04, 0.01, 0.01, 5)


# ---- the divisor rule -------------------------------------------------------------------------------------------------------------------
def _owners(pr, P):
    owner = np.asarray(Engine.partition_nodes(pr["N"], P, mesh_pos=pr["pos"]))
    assert sorted(set(owner.tolist())) == list(range(P))
    return owner


@pytest.mark.parametrize("P", [2, 3])
def test_per_owner_save_sums_over_the_global_count_are_the_whole_mesh_loss(lib_built, P):
    """The save term of the solver loss as a partitioned call forms it -- every owner's sum of ((gt - x) .* loss_scale) .^ 2 .* val_mask over
    its own nodes, the owners' sums added in ascending rank order, ONE division by n_saves * N * O of the whole mesh -- against the
    whole-mesh loss of the float64 drivers (Euler: solver_adjoint_ref, Tsit5: tsit5_adjoint_ref) on the oracle's right-hand side."""
    pr = case()
    gt, vm, ns, N = pr["gt"], pr["vm"], pr["ns"], pr["N"]
    owner = _owners(pr, P)
    rhs, _, _ = oracle_fns(pr)
    no_vjp = lambda x, lam: (np.zeros_like(x), np.zeros(1))      # noqa: E731  (the loss alone)
    _, loss_e, pred_e, _ = sar.euler_adjoint(rhs, no_vjp, gt[0], gt, 0.0, 0.04, 0.01, 0.01, 5, val_mask=vm, loss_scale=ns)
    step_t, step_h, save_step, _ = tar.fixed_steps(0.0, 0.04, 0.01, 0.01, 5)
    _, loss_t, pred_t, _ = tar.tsit5_adjoint(rhs, no_vjp, gt[0], gt, step_t, step_h, save_step, 0.01, val_mask=vm, loss_scale=ns)
    for loss, pred in ((loss_e, pred_e), (loss_t, pred_t)):
        per_node = save_loss_terms(gt, pred, ns, vm)
        folded = rank_ordered(owner, per_node, P) / (5 * N * 2)
        assert abs(folded - loss) <= 1e-12 * abs(loss), (folded, loss)
        # a rank's own count as the divisor is a different number: the rule is the global one
        own = sum(per_node[owner == k].sum() / (5 * max(int((owner == k).sum()), 1) * 2) for k in range(P))
        assert abs(own - loss) > 1e-3 * abs(loss)


class _CannedEngine:
    """Engine.rollout_eval's contract in float64 over a canned prediction, the whole mesh at once (reference_api.validation_step's engine)"""

    def __init__(self, pred):
        self.pred = pred

    def rollout_eval(self, solver, x0, node_type_onehot, ef_raw, gt, t0, t1, saves_dt, n_saves, sel=None, sel_index_base=0, **kw):
        q = (self.pred[:n_saves].astype(np.float64) - np.asarray(gt[:n_saves], np.float64)) ** 2
        flat = q.mean(axis=0).reshape(-1)
        return {"val_loss": float(flat[np.asarray(sel, np.int64) - sel_index_base].mean()), "pred": None}


@pytest.mark.parametrize("P", [2, 3])
def test_val_loss_with_a_duplicate_and_an_empty_share(lib_built, P):
    """validation_step's mean(error[mask]) on partitions: every entry of sel counts on the rank that owns its node, as often as it is
    listed; the owners' sums fold in rank order; the divisor is len(sel).  sel lists one entry twice and no element of one rank's nodes."""
    pr = case()
    gt, N, O = pr["gt"], pr["N"], 2
    owner = _owners(pr, P)
    rng = np.random.default_rng(8)
    pred = (gt + 0.1 * rng.standard_normal(gt.shape)).astype(F32)
    # the reference's mask is a vector of node indices that indexes the O x N matrix LINEARLY: entry m is element m of [N][O], which
    # belongs to node m // O -- so "no node of the last rank" is a statement about m // O
    skip = int(owner[0])                                                           # the rank whose share stays empty
    nodes = np.nonzero(owner[np.arange(N) // O] != skip)[0]
    assert 0 < nodes.size < N
    mask1 = np.concatenate([nodes[::7], nodes[7:8]]).astype(np.int32) + 1          # 1-based, as `findall` gives them; one entry twice
    assert np.unique(mask1).size == mask1.size - 1
    want, _, _ = ra.validation_step(_CannedEngine(pred), gt, None, None, (0.0, 0.01, 0.04), mask1, solver="Euler", solver_dt=0.01,
                                    mask_index_base=1)
    acc = ((pred.astype(np.float64) - gt) ** 2).sum(axis=0) / 5.0                  # [N][O]: mse_time before it is rounded
    li = mask1.astype(np.int64) - 1                                                # LINEAR indices into [N][O]
    shares = [li[owner[li // O] == k] for k in range(P)]
    assert shares[skip].size == 0 and sum(s.size for s in shares) == li.size
    total = 0.0
    for k in range(P):
        part = 0.0
        for j in shares[k]:
            part += float(acc.reshape(-1)[j])
        total = total + part
    got = total / li.size
    assert abs(got - want) <= 1e-12 * abs(want), (got, want)
