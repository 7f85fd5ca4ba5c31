"""mgn_rollout_eval (Engine.rollout_eval): mgn_rollout's solve with the errors against the ground truth reduced on the device --
_validation_step's `mean(error[mask])` and eval_network!'s per-save error (reference src/strategies.jl:111-134,
src/MeshGraphNets.jl:609-635).  The solve is checked bit for bit against Engine.rollout, the reductions against float64 NumPy over the
call's OWN prediction (which isolates them from the solve).  Run on the MI355X box with `-m gpu`.

Tolerances.  The device forms (x - gt) and its square in double from the fp32 values, exactly as NumPy does on float64 copies, and
adds in double; only the order of the additions differs (at most 8 saves and 2640 elements here, each addition within 2^-53): mse_save
and val_loss agree to 1e-12 relative.  mse_time is that double mean rounded once to float: 2^-23 relative."""
import numpy as np
import pytest
import torch   # before the engine's first HIP call (device-array test), or torch finds no GPU afterwards

import mgn_oracle as orc
from mgn_amd import MgnError, _capi, synth
from util import cfg_dict, engine_for, make_params, renumbered, scatter_labels

pytestmark = pytest.mark.gpu

SDT = 0.01


def problem(kind, O=2, K=5, scramble=False, L=64, mps=2):
    """Built like problem() of tests/test_gpu_solver_train.py.  kind "cyl": synth.mesh_cyl(..., 150), fewer rows than one block of
    k_save_error; "grid": a 40 x 33 grid, 1320 nodes = five full blocks and a ragged sixth.  O = 3: an odd row width (scalar loads)."""
    cfg = cfg_dict(Fn=O + 7, O=O, L=L, mps=mps)
    if kind == "cyl":
        pos, cells, node_type, vel = synth.mesh_cyl(1234, 150)
    else:
        pos, cells = synth.grid_mesh(40, 33, 1234)
        rng0 = np.random.default_rng(1)
        node_type = rng0.choice([0, 1, 4, 5, 6], pos.shape[0], p=[0.8, 0.05, 0.05, 0.05, 0.05]).astype(np.int32)
        vel = rng0.standard_normal((pos.shape[0], 2)).astype(np.float32)
    if O > 2:
        vel = np.concatenate([vel, 0.5 * vel[:, :1] - vel[:, 1:2]] + [vel[:, :1]] * (O - 3), axis=1).astype(np.float32)
    s, r = synth.cells_to_edges(cells)
    if scramble:
        pos, s, r, perm = scatter_labels(pos, s, r, seed=3)
        inv = np.argsort(perm)
        node_type, vel = node_type[inv], vel[inv]
    N = pos.shape[0]
    rng = np.random.default_rng(6)
    onehot = orc.one_hot(node_type, 7, 0).astype(np.float32)
    ef_raw = orc.edge_features(pos, s, r).astype(np.float32)
    # every element of every frame differs from the prediction (a relative bound on an exact zero would say nothing): a floor under
    # |vel| (wall nodes have none), and an x0 that is not gt[0]
    vel = np.where(np.abs(vel) < 0.05, 0.05, vel).astype(np.float32)
    gt = (vel[None] * (1.0 + 0.05 * rng.standard_normal((K + 1, N, O)))).astype(np.float32)
    x0 = (gt[0] * (1.0 + 0.02 * rng.standard_normal((N, O)))).astype(np.float32)
    n_norm = orc.NormMeanStd(np.array([1.0, 0.1, 0.3][:O]), np.array([0.4, 0.2, 0.3][:O]))
    o_norm = orc.NormMeanStd(np.array([0.01, -0.02, 0.03][:O]), np.array([5.0, 4.0, 6.0][:O]))
    e_norm = orc.NormMeanStd(ef_raw.mean(0), ef_raw.std(0))
    ns, nsh = n_norm.affine(O)
    ts, tsh = orc.NormMinMax(0.0, 1.0).affine(7)
    es, esh = e_norm.affine(3)
    eng = engine_for(cfg)
    eng.set_params(make_params(cfg).astype(np.float32))
    eng.set_graph(s, r, N)
    eng.set_norms(node=(np.concatenate([ns, ts]), np.concatenate([nsh, tsh])), edge=(es, esh), out=(o_norm.std, o_norm.mean))
    return dict(eng=eng, N=N, O=O, K=K, onehot=onehot, ef_raw=ef_raw, gt=gt, x0=x0, node_type=node_type, rng=rng,
                vm=np.isin(node_type, [0, 5]).astype(np.float32))


_PROBLEMS = {}


def get(kind, O=2, scramble=False):
    key = (kind, O, scramble)
    if key not in _PROBLEMS:
        _PROBLEMS[key] = problem(kind, O=O, scramble=scramble)
    return _PROBLEMS[key]


def solve_args(P, solver):
    ns = P["K"] + 1
    return (solver, P["x0"], P["onehot"], P["ef_raw"]), dict(t0=0.0, t1=SDT * (ns - 1), saves_dt=SDT, n_saves=ns,
                                                              dt=SDT if solver == "Euler" else 0.0, val_mask=P["vm"], inflow_rule="tolerant")


def run_eval(P, solver, gt=None, **kw):
    a, k = solve_args(P, solver)
    k.update(kw)
    return P["eng"].rollout_eval(*a[:4], P["gt"] if gt is None else gt, k.pop("t0"), k.pop("t1"), k.pop("saves_dt"), k.pop("n_saves"), **k)


def run_rollout(P, solver, **kw):
    a, k = solve_args(P, solver)
    k.update(kw)
    return P["eng"].rollout(*a, k.pop("t0"), k.pop("t1"), k.pop("saves_dt"), k.pop("n_saves"), **k)


def np_reference(pred, gt, sel=None, base=0):
    """strategies.jl:131-133 and MeshGraphNets.jl:615-619 in float64: (mse_save [n_saves][O], mse_time [N][O], mean(error[sel]))."""
    q = (pred.astype(np.float64) - gt[:pred.shape[0]].astype(np.float64)) ** 2
    mse_time = q.mean(axis=0)
    flat = mse_time.reshape(-1)                        # row-major [N][O] == Julia's column-major O x N: linear indices agree
    return q.mean(axis=1), mse_time, float(flat.mean() if sel is None else flat[np.asarray(sel, np.int64) - base].mean())


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))


def assert_same_results(r, q):
    assert np.float64(r["val_loss"]).tobytes() == np.float64(q["val_loss"]).tobytes(), (r["val_loss"], q["val_loss"])
    assert same_bits(r["mse_save"], q["mse_save"])
    assert same_bits(r["mse_time"], q["mse_time"])


def assert_reductions(r, gt, sel=None, base=0):
    ms, mt, vl = np_reference(r["pred"], gt, sel, base)
    assert (mt > 0).all() and (ms[1:] > 0).all()
    e_save = float(np.max(np.abs(r["mse_save"] - ms) / np.where(ms > 0, ms, 1.0)))
    e_time = float(np.max(np.abs(r["mse_time"].astype(np.float64) - mt) / mt))
    e_val = abs(r["val_loss"] - vl) / vl
    print(f"rel err: mse_save {e_save:.3e}  mse_time {e_time:.3e} (2^-23 = {2.0 ** -23:.3e})  val_loss {e_val:.3e}")
    assert r["mse_time"].dtype == np.float32 and r["mse_save"].dtype == np.float64
    assert e_save <= 1e-12, e_save
    assert e_time <= 2.0 ** -23, e_time
    assert e_val <= 1e-12, e_val


@pytest.mark.parametrize("kind", ["cyl", "grid"])
@pytest.mark.parametrize("solver", ["Euler", "Tsit5"])
def test_prediction_is_rollouts_bit_for_bit_and_repeatable(kind, solver):
    P = get(kind)
    ref, st = run_rollout(P, solver)
    r = run_eval(P, solver, want_pred=True)
    assert same_bits(r["pred"], ref)
    assert r["stats"] == st and st["n_rhs"] > 0
    q = run_eval(P, solver, want_pred=True)
    assert same_bits(q["pred"], r["pred"]) and q["stats"] == r["stats"]
    assert_same_results(r, q)


@pytest.mark.parametrize("kind,O,solver", [("cyl", 2, "Euler"), ("grid", 2, "Tsit5"), ("cyl", 3, "Euler"), ("grid", 3, "Euler")])
def test_reductions_match_float64_numpy_over_the_calls_own_prediction(kind, O, solver):
    P = get(kind, O)
    r = run_eval(P, solver, want_pred=True)
    assert np.isfinite(r["pred"]).all()
    assert_reductions(r, P["gt"])


@pytest.mark.parametrize("kind,O", [("cyl", 2), ("grid", 2), ("cyl", 3)])
def test_without_the_solution_the_results_are_the_same_bits(kind, O):
    P = get(kind, O)
    sel = P["rng"].integers(0, P["N"] * O, 40)
    with_out = run_eval(P, "Euler", want_pred=True, sel=sel)
    without = run_eval(P, "Euler", want_pred=False, sel=sel)
    assert without["pred"] is None
    assert_same_results(with_out, without)
    assert without["stats"] == with_out["stats"]


@pytest.mark.parametrize("kind,scramble", [("cyl", False), ("grid", True)])
def test_ground_truth_that_is_the_inflow_data_is_not_a_different_result(kind, scramble):
    P = get(kind, scramble=scramble)
    im = ((P["node_type"] == 4) | (P["node_type"] == 1)).astype(np.uint8)
    assert im.any()
    gt = P["gt"]
    aliased = run_eval(P, "Euler", gt=gt, inflow_mask=im, inflow_data=gt, want_pred=True)
    copied = run_eval(P, "Euler", gt=gt.copy(), inflow_mask=im, inflow_data=gt, want_pred=True)
    assert same_bits(aliased["pred"], copied["pred"])
    assert_same_results(aliased, copied)
    assert_same_results(aliased, run_eval(P, "Euler", gt=gt, inflow_mask=im, inflow_data=gt))      # and with out = NULL
    ref, _ = run_rollout(P, "Euler", inflow_mask=im, inflow_data=gt)
    assert same_bits(aliased["pred"], ref)


@pytest.mark.parametrize("solver", ["Euler", "Tsit5"])
def test_renumbered_graph_answers_in_the_callers_order(solver):
    P = get("grid", scramble=True)
    assert renumbered(P["eng"])
    N, O = P["N"], P["O"]
    mask = np.nonzero(np.isin(P["node_type"], [0, 5]))[0].astype(np.int32)
    sel = np.concatenate([mask + 1, mask[:1] + 1, [N * O]]).astype(np.int32)      # 1-based, a duplicate, the last element
    r = run_eval(P, solver, want_pred=True, sel=sel, sel_index_base=1)
    ref, _ = run_rollout(P, solver)
    assert same_bits(r["pred"], ref)
    assert_reductions(r, P["gt"], sel, 1)
    assert_same_results(r, run_eval(P, solver, sel=sel, sel_index_base=1))


def test_sel_is_linear_indexing_of_the_error_matrix():
    P = get("grid")
    N, O = P["N"], P["O"]
    none = run_eval(P, "Euler", want_pred=True)
    assert_reductions(none, P["gt"])                                        # n_sel = 0: the mean over all N * O elements
    every = run_eval(P, "Euler", sel=np.arange(N * O, dtype=np.int32))
    assert abs(every["val_loss"] - none["val_loss"]) <= 1e-12 * none["val_loss"]
    mask = np.nonzero(np.isin(P["node_type"], [0, 5]))[0].astype(np.int32)  # the reference's node indices
    r = run_eval(P, "Euler", want_pred=True, sel=mask)
    assert_reductions(r, P["gt"], mask)                                     # mean(error[mask]): elements mask[i] of [N][O]
    _, mt, _ = np_reference(r["pred"], P["gt"])
    rows = float(mt[mask].mean())                                           # "all components of node mask[i]" is another number
    assert abs(r["val_loss"] - rows) > 1e-6 * rows
    dup = run_eval(P, "Euler", want_pred=True, sel=np.concatenate([mask, mask[:3]]))
    assert_reductions(dup, P["gt"], np.concatenate([mask, mask[:3]]))       # duplicates count twice


def test_ground_truth_and_mse_time_on_the_device():
    P = get("grid")
    host = run_eval(P, "Euler", sel=np.arange(7, dtype=np.int32))
    gt_dev = torch.from_numpy(P["gt"]).cuda()
    mt_dev = torch.zeros((P["N"], P["O"]), dtype=torch.float32, device="cuda")
    dev = run_eval(P, "Euler", gt=gt_dev, sel=np.arange(7, dtype=np.int32), mse_time_out=mt_dev)
    torch.cuda.synchronize()
    assert dev["mse_time"] is mt_dev
    dev["mse_time"] = mt_dev.cpu().numpy()
    assert_same_results(host, dev)


def test_refusals_leave_the_engine_usable():
    P = get("cyl")
    N, O, ns = P["N"], P["O"], P["K"] + 1
    before = run_eval(P, "Euler")
    cases = [(dict(gt=P["gt"][:ns - 1]), "Euler", _capi.MGN_E_ARG),                         # n_gt < n_saves
             (dict(sel=np.array([0, N * O], np.int32)), "Euler", _capi.MGN_E_ARG),         # one past the end
             (dict(sel=np.array([0], np.int32), sel_index_base=1), "Euler", _capi.MGN_E_ARG),
             (dict(sel=np.array([1], np.int32), sel_index_base=2), "Euler", _capi.MGN_E_ARG),
             (dict(abstol=0.0), "Tsit5", _capi.MGN_E_ARG),
             (dict(inflow_mask=np.ones(N, np.uint8)), "Euler", _capi.MGN_E_ARG)]            # mgn_rollout's: mask without data
    for kw, solver, code in cases:
        with pytest.raises(MgnError) as ei:
            run_eval(P, solver, **kw)
        assert ei.value.code == code, (kw, ei.value)
        assert "mgn_rollout_eval" in str(ei.value)
    assert_same_results(before, run_eval(P, "Euler"))
