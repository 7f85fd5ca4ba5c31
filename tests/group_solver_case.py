"""The fixture of tests/test_group_solver_host.py and tests/test_gpu_group_solver_train.py (a helper of the tests, not a test): the 40 x 33
grid of test_gpu_partitioned_step.grid_case (1320 nodes) with the norms, one-hot node types, raw edge features, ground truth, val_mask
and loss scale built as test_gpu_solver_train.problem(grid=(40, 33)) builds them, without an engine -- the host test has no device.
L = 64, mps = 2, hidden_layers = 2 unless asked otherwise: the smallest shape in which every rank of P = 2, 3 and 4 has boundary and
interior rows, with more than one processor step so that the reverse halo exchange runs between two node MLPs."""
import functools

import numpy as np

import mgn_oracle as orc
from mgn_amd import synth
from util import cfg_dict, make_params, scatter_labels

F32 = np.float32


@functools.lru_cache(maxsize=None)
def case(L=64, mps=2, hidden_layers=2, K=4, scattered=False, seed=6):
    """Read-only.  K + 1 ground-truth frames (K steps of 0.01, K + 1 saves)."""
    cfg = cfg_dict(L=L, mps=mps)
    cfg["hidden_layers"] = hidden_layers
    pos, cells = synth.grid_mesh(40, 33, 9)
    rng0 = np.random.default_rng(1)
    node_type = rng0.choice([0, 1, 4, 5, 6], pos.shape[0], p=[0.8, 0.05, 0.05, 0.05, 0.05]).astype(np.int32)
    vel = rng0.standard_normal((pos.shape[0], 2)).astype(F32)
    s, r = synth.cells_to_edges(cells)
    if scattered:      # the same mesh under arbitrary node labels: the engine renumbers
        pos, s, r, perm = scatter_labels(pos, s, r, seed=3)
        inv = np.argsort(perm)
        node_type, vel = node_type[inv], vel[inv]
    N = pos.shape[0]
    rng = np.random.default_rng(seed)
    onehot = orc.one_hot(node_type, 7, 0).astype(F32)
    ef_raw = orc.edge_features(pos, s, r).astype(F32)
    gt = (vel[None] * (1.0 + 0.05 * rng.standard_normal((K + 1, N, 2)))).astype(F32)
    P = dict(cfg=cfg, pos=pos, s=np.ascontiguousarray(s), r=np.ascontiguousarray(r), N=N, E=int(s.size), K=K, onehot=onehot, ef_raw=ef_raw, gt=gt,
             node_type=node_type, n_norm=orc.NormMeanStd(np.array([1.0, 0.1]), np.array([0.4, 0.2])), t_norm=orc.NormMinMax(0.0, 1.0),
             e_norm=orc.NormMeanStd(ef_raw.mean(0), ef_raw.std(0)), o_norm=orc.NormMeanStd(np.array([0.01, -0.02]), np.array([5.0, 4.0])),
             vm=np.isin(node_type, [0, 5]).astype(F32))
    P["ps"] = make_params(cfg).astype(F32)
    ns, nsh = P["n_norm"].affine(2)
    ts, tsh = P["t_norm"].affine(7)
    es, esh = P["e_norm"].affine(3)
    P["ns"] = ns
    P["norms"] = dict(node=(np.concatenate([ns, ts]), np.concatenate([nsh, tsh])), edge=(es, esh), out=(P["o_norm"].std, P["o_norm"].mean))
    P["inflow_mask"] = ((node_type == 4) | (node_type == 1)).astype(np.uint8)
    P["frames"] = (gt[0][None] * (1.0 + 0.2 * rng.standard_normal((K + 1, N, 2)))).astype(F32)
    P["cont_target"] = (gt[-1] + 0.3 * rng.standard_normal(gt[-1].shape)).astype(F32)
    for v in P.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return P


def setup(e, P):
    """parameters, normalisers and graph of the case on an Engine or a GroupEngine"""
    e.set_params(P["ps"])
    e.set_norms(**P["norms"])
    e.set_graph(P["s"], P["r"], P["N"], mesh_pos=P["pos"])


def oracle_fns(P, inflow=False, val_mask=True):
    """(rhs, vjp, rhs_at) of the float64 oracle on the case, as test_gpu_solver_train.oracle_fns; val_mask False: a right-hand side
    without val_mask (all ones), for the calls that pass none"""
    args = (P["onehot"], P["ef_raw"], P["s"], P["r"], P["n_norm"], P["t_norm"], P["e_norm"], P["o_norm"])
    vm = P["vm"] if val_mask else np.ones_like(P["vm"])
    vm2 = vm[:, None].astype(np.float64)
    ps, im, frames = P["ps"], P["inflow_mask"].astype(bool), P["frames"]

    def rhs(x):
        return orc.ode_rhs(ps, P["cfg"], x, *args, vm2)

    def rhs_at(x, fr):
        if fr is None or not inflow:
            return rhs(x)
        return orc.ode_rhs(ps, P["cfg"], x, *args, vm2, inflow_mask=im, inflow_values=frames[fr])

    def vjp(x, lam):
        return orc.ode_vjp(ps, P["cfg"], x, *args, vm, lam)[:2]

    return rhs, vjp, rhs_at


def save_loss_terms(gt, pred, loss_scale, val_mask):
    """[N] float64: every node's sum over saves and components of ((gt - pred) .* loss_scale) .^ 2 .* val_mask -- the numerator of the save
    term of the solver loss, node by node"""
    q = ((np.asarray(gt, np.float64) - np.asarray(pred, np.float64)) * np.asarray(loss_scale, np.float64).reshape(1, 1, -1)) ** 2
    return (q * np.asarray(val_mask, np.float64).reshape(1, -1, 1)).sum(axis=(0, 2))


def rank_ordered(owner, per_node, P):
    """the ranks' sums of per_node over the nodes they own (running sums, no pairwise trick), added in ascending rank order"""
    total = 0.0
    for k in range(P):
        part = 0.0
        for v in per_node[owner == k]:
            part += float(v)
        total = total + part
    return total
