"""Every entry point at the edges of the width rule (include/mgn_hip.h, mgn_config "Widths"; cases in tests/width_cases.py): widths of
1, of exactly L, across the 32-column tile, O >= 5 and O = Fn = L where the training kernels compute, and widths above L where only
inference does.  Everything is compared with the float64 oracle or a float64 NumPy restatement; two engine results are compared only
where "bits" says so.  Run on the MI355X box with `-m gpu`.

Unless a test says otherwise: util.small_mesh(9, 7) (63 nodes, 316 edges), mps = 2, orc.init_params(seed=1234, ln_jitter=0.1),
standard-normal inputs.  The bounds are the project's own, under the names they carry in the files they come from; none of them
is widened for width.

Largest err / bound per test on the MI355X, over the cases of the test, and the case that gave it (every test prints its figures,
`pytest -s`):
  forward, default dispatch            out 0.0099 (full32)
  forward, 2083 nodes at 8 test CUs    out 0.013 (full32)
  staged encode / decode above L       of TOL_STEP: encode v 0.022, e 0.016 (wide 65/3/2 at L 64), decode 0.011 (wide 33/64/33 at L 32)
  fused RHS, both forms (same bits)    0.0066 (edge128)
  rollout_eval, Euler                  mse_save 8.4e-4 (wide 33/64/33 at L 32), mse_time 0.49 (full32), val_loss 2.3e-4 (cross64)
  rollout_eval, fixed-step Tsit5       mse_save 6.6e-4, mse_time 0.49 (both wide 33/64/33 at L 32), val_loss 2.1e-4 (edge128)
  step                                 loss 0.0089 (full64h3), gradient 0.0060 (full32)
  ode_vjp                              dxdt 0.0075 (edge128), rows 0.0025, row L2 1.1e-4, gradient L2 1.0e-4, tensors 5e-5
  forward_vjp                          out 0.0064 (edge128), rows 0.0021, row L2 1.1e-4, gradient L2 1.4e-4, tensors 6e-5
  datapoint path                       normalised nf / ef against build_graph: 2.0 ulp, ON the bound of 2.0, at every case (below);
                                       everything else there is compared bit for bit
  solver_grad                          loss 4.1e-4 (out32), gradient 4e-5, saves 8.6e-4 (cross64)
  whole-array LayerNorm                out 0.0056, loss 0.0061, gradient 0.0020 (all full32)
  two edge sets, Fe2 = L               out 0.0069, loss 0.0056, gradient 0.0048
  two partitions (cross64)             out 0.0049, loss 0.0012, gradient 0.0039
  width sweep                          out 0.0066 (draw 0), loss 0.010 (draw 1), gradient L2 1.9e-4 of 2e-3 (draw 1): no draw took the
                                       fp32 cross-check
Two figures lie near their bounds, both by construction.  mse_time is one rounding of a double to float: at most half of 2^-23.  The
datapoint path's 2 ulp is the bound tests/test_gpu_step_datapoint.py::test_assembly_against_the_mirror holds the same comparison to, in
the measure of train_checks.affine_ulps: the device evaluates x * (1 / std) + (-mean / std), the mirror (x - mean) / std, and the
difference is counted in spacings of float32 at the largest of |x / std|, |mean / std| and the result.  Three roundings on one side
(the reciprocal, the shift, the sum) and two on the other can in principle add up to more than 2 such spacings, so the bound is not a
theorem; with up to 316 x 128 edge values per datapoint (edge128) against that file's 240 x 3 the largest difference met is 2 spacings.  The inputs are seeded and the engine is deterministic: the figure does not move
from run to run.  Every other figure stays below 2 % of its bound.  No case exposed a defect: the widths in range compute what the
oracle computes, and inference does above L.
"""
import numpy as np
import pytest
import torch   # before the engine's first HIP call, or torch finds no GPU afterwards

import mgn_amd
import mgn_oracle as orc
import solver_adjoint_ref as sar
import width_cases as wc
from mgn_amd import GroupEngine, MgnError, _capi, synth
from mgn_amd import reference_api as ra
from train_checks import TOL_GRAD, TOL_LOSS, affine_ulps, check_grads
from util import TOL_15, TOL_STEP, rel_max, set_num_cus

pytestmark = pytest.mark.gpu

F32 = np.float32
IN_RANGE = list(wc.IN_RANGE)


def ids(cases):
    return [wc.case_id(c) for c in cases]


_live = []


def engine_of(cfg, **kw):
    eng = mgn_amd.Engine(cfg["Fn"], cfg["Fe"], cfg["O"], cfg["L"], cfg["hidden_layers"], cfg["mps"], Fe2=cfg.get("Fe2"), **kw)
    _live.append(eng)
    return eng


@pytest.fixture(autouse=True)
def close_engines():
    """no handle of this file (its streams, its captured graphs) outlives its test"""
    yield
    while _live:
        _live.pop().close()


def engine_on(P, norms=False, **kw):
    eng = engine_of(P.cfg, **kw)
    eng.set_params(P.ps)
    eng.set_graph(P.s, P.r, P.N)
    if norms:
        eng.set_norms(node=P.n_norm, edge=P.e_norm, out=P.o_norm)
    return eng


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def rel_l2(a, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.linalg.norm(np.asarray(a, np.float64) - ref) / max(np.linalg.norm(ref), 1e-30))


def report(test, case, **ratios):
    """err / bound of every checked quantity, for the table in the module docstring"""
    print("WIDTHS %s %s %s" % (test, wc.case_id(case), " ".join("%s=%.3g" % kv for kv in ratios.items())))


def check_step(eng, P, test, case, set2=None):
    """mgn_step against the oracle at TOL_LOSS / TOL_GRAD; a second call returns the same bits"""
    gs, loss = eng.step(P.nf, P.ef, P.target, P.mask)
    ref, ref_loss = orc.step_grads(P.ps, P.cfg, P.nf, P.ef, P.s, P.r, P.target, P.mask, set2=set2)
    e_loss = abs(loss - ref_loss) / abs(ref_loss)
    report(test, case, loss=e_loss / TOL_LOSS)
    assert e_loss <= TOL_LOSS, (loss, ref_loss)
    report(test, case, grad=check_grads(gs, ref, P.cfg)[1] / TOL_GRAD)
    gs2, loss2 = eng.step(P.nf, P.ef, P.target, P.mask)
    assert loss2 == loss and same_bits(gs, gs2)
    return gs, loss


# ---- 1. forward ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", wc.ALL_FORWARD, ids=ids(wc.ALL_FORWARD))
def test_forward(case):
    P = wc.problem(case)
    err = rel_max(engine_on(P).forward(P.nf, P.ef), orc.forward(P.ps, P.cfg, P.nf, P.ef, P.s, P.r))
    report("forward", case, out=err / TOL_15)
    assert err <= TOL_15, err


@pytest.mark.parametrize("case", wc.ALL_FORWARD, ids=ids(wc.ALL_FORWARD))
def test_forward_above_the_cooperative_range(case):
    """2083 nodes, 4137 edges at a test CU count of 8: the resident encoder / decoder launches of eight waves, whose waves walk a
    second tile (tests/test_gpu_encdec_stages.py, "resident8")"""
    P = wc.problem(case, "resident8")
    old = set_num_cus(8)
    assert old >= 0
    try:
        out = engine_on(P).forward(P.nf, P.ef)
    finally:
        set_num_cus(old)
    err = rel_max(out, orc.forward(P.ps, P.cfg, P.nf, P.ef, P.s, P.r))
    report("forward_resident8", case, out=err / TOL_15)
    assert err <= TOL_15, err


@pytest.mark.parametrize("case", wc.WIDE, ids=ids(wc.WIDE))
def test_staged_encode_and_decode_above_L(case):
    """mgn_fwd_upload / _encode and mgn_fwd_decode / _download on their own, as tests/test_gpu_encdec_stages.py runs them, at its bound:
    the first layers over more than L input features, the decoder's head over more than L outputs"""
    P = wc.problem(case)
    h, L = P.cfg["hidden_layers"], P.cfg["L"]
    W = orc._unpack(P.ps, P.cfg, np.float64)
    eng = engine_on(P)
    rv, re = orc.encode(W, P.nf.astype(np.float64), P.ef.astype(np.float64), h)
    eng.fwd_upload(P.nf, P.ef)
    eng.fwd_encode()
    v, e = eng.latents_export()
    rng = np.random.default_rng(3)
    v1, e1 = rng.standard_normal((P.N, L)).astype(F32), rng.standard_normal((P.E, L)).astype(F32)
    eng.latents_import(v1, e1)
    eng.fwd_decode()
    out = eng.fwd_download()
    ref = orc.decode(W, v1.astype(np.float64), h)
    report("staged", case, v=rel_max(v, rv) / TOL_STEP, e=rel_max(e, re) / TOL_STEP, decode=rel_max(out, ref) / TOL_STEP)
    assert rel_max(v, rv) <= TOL_STEP and rel_max(e, re) <= TOL_STEP
    assert out.shape == (P.N, P.cfg["O"]) and rel_max(out, ref) <= TOL_STEP


# ---- 2. the fused right-hand side ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", wc.ALL_FORWARD, ids=ids(wc.ALL_FORWARD))
def test_fused_rhs_both_forms(case):
    P = wc.problem(case)
    ref = wc.rhs_reference(P)
    eng = engine_on(P, norms=True)
    one_shot = eng.ode_step(P.x, P.onehot, P.ef, P.vm)
    eng.set_static(P.onehot, P.ef, P.vm)
    resident = eng.ode_step(P.x)
    report("fused_rhs", case, one_shot=rel_max(one_shot, ref) / TOL_15, resident=rel_max(resident, ref) / TOL_15)
    assert rel_max(one_shot, ref) <= TOL_15 and rel_max(resident, ref) <= TOL_15
    assert same_bits(one_shot, resident)
    assert np.all(one_shot[P.vm == 0] == 0) and np.abs(one_shot[P.vm == 1]).min() > 0


# ---- 3. rollout and its reductions -----------------------------------------------------------------------------------------------
SDT = 0.01
ROLLOUT_CASES = ["min", "full32", "cross64", "edge128", wc.WIDE[0]]


def np_reductions(pred, gt, sel):
    """strategies.jl:131-133 and MeshGraphNets.jl:615-619 in float64: (mse_save [n_saves][O], mse_time [N][O], mean(error[sel]))"""
    q = (pred.astype(np.float64) - gt[:pred.shape[0]].astype(np.float64)) ** 2
    mse_time = q.mean(axis=0)
    flat = mse_time.reshape(-1)
    return q.mean(axis=1), mse_time, float(flat.mean() if sel is None else flat[np.asarray(sel, np.int64)].mean())


@pytest.mark.parametrize("solver", ["Euler", "Tsit5-fixed"])
@pytest.mark.parametrize("case", ROLLOUT_CASES, ids=ids(ROLLOUT_CASES))
def test_rollout_eval_and_its_reductions(case, solver):
    P = wc.problem(case)
    N, O = P.N, P.cfg["O"]
    euler = solver == "Euler"
    n_saves = 4 if euler else 3
    rng = np.random.default_rng(17 + n_saves)
    gt = rng.standard_normal((n_saves + 1, N, O)).astype(F32)
    frames = rng.standard_normal((n_saves + 1, N, O)).astype(F32)            # the inflow data: not the ground truth
    im = np.zeros(N, np.uint8)
    im[[0, 7, 20, 41, N - 1]] = 1
    eng = engine_on(P, norms=True)
    args = ("Euler" if euler else "Tsit5", P.x, P.onehot, P.ef)
    grid = (0.0, SDT * (n_saves - 1), SDT, n_saves)
    kw = dict(dt=SDT if euler else SDT / 2, val_mask=P.vm, inflow_mask=im, inflow_data=frames, inflow_rule="tolerant", adaptive=False)
    ref, stats = eng.rollout(*args, *grid, **kw)
    assert np.isfinite(ref).all() and stats["n_rhs"] > 0 and not same_bits(ref[-1], ref[0])
    sels = (None, np.array([3, N * O - 1, 3, 5 * O + (O - 1), 3, 0], np.int32))        # n_sel = 0; a repeated index, the last element
    for sel in sels:
        r = eng.rollout_eval(*args[:4], gt, *grid, sel=sel, want_pred=True, **kw)
        assert same_bits(r["pred"], ref) and r["stats"] == stats
        ms, mt, vl = np_reductions(r["pred"], gt, sel)
        assert (mt > 0).all() and (ms > 0).all()
        assert r["mse_time"].dtype == np.float32 and r["mse_save"].dtype == np.float64 and r["mse_save"].shape == (n_saves, O)
        e_save = float(np.max(np.abs(r["mse_save"] - ms) / ms))
        e_time = float(np.max(np.abs(r["mse_time"].astype(np.float64) - mt) / mt))
        e_val = abs(r["val_loss"] - vl) / vl
        report("rollout_eval_" + solver, case, save=e_save / 1e-12, time=e_time / 2.0 ** -23, val=e_val / 1e-12)
        assert e_save <= 1e-12, e_save
        assert e_time <= 2.0 ** -23, e_time          # the double mean rounded once to float
        assert e_val <= 1e-12, e_val


# ---- 4. the training step --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", IN_RANGE)
def test_step(case):
    P = wc.problem(case)
    check_step(engine_on(P), P, "step", case)


# ---- 5. the pullbacks ------------------------------------------------------------------------------------------------------------
VJP_CASES = ["min", "out32", "cross64", "edge128"]


def check_pullback(test, case, rows, ref_rows, gs, ref_gs, cfg):
    """the criterion of tests/test_gpu_training_step.py::test_ode_vjp_matches_oracle_and_ode_step (ReLU kinks: all but 2 % of the rows
    within TOL_GRAD, small relative L2 errors overall, every parameter tensor within 2e-2)"""
    row_err = np.abs(rows - ref_rows).max(1) / np.abs(ref_rows).max()
    q = float(np.quantile(row_err, 0.98))
    report(test, case, rows98=q / TOL_GRAD, rows_l2=rel_l2(rows, ref_rows) / 5e-3, gs_l2=rel_l2(gs, ref_gs) / 5e-3)
    assert q <= TOL_GRAD, q
    assert rel_l2(rows, ref_rows) <= 5e-3 and rel_l2(gs, ref_gs) <= 5e-3
    report(test, case, tensors=check_grads(gs, ref_gs, cfg, tol=2e-2)[1] / 2e-2)


@pytest.mark.parametrize("case", VJP_CASES)
def test_ode_vjp(case):
    P = wc.problem(case)
    eng = engine_on(P, norms=True)
    xbar, gs, dxdt = eng.ode_vjp(P.x, P.onehot, P.ef, P.lam, val_mask=P.vm, want_dxdt=True)
    oh = P.onehot if P.onehot is not None else np.zeros((P.N, 0), F32)
    rx, rg, rf = orc.ode_vjp(P.ps, P.cfg, P.x, oh, P.ef, P.s, P.r, *wc.oracle_norms(P), P.vm, P.lam)
    report("ode_vjp", case, dxdt=rel_max(dxdt, rf) / 1e-4)
    assert rel_max(dxdt, rf) <= 1e-4
    assert rel_max(rf, wc.rhs_reference(P)) <= 1e-12                 # (the oracle's composition is the restatement of test 2)
    check_pullback("ode_vjp", case, xbar, rx, gs, rg, P.cfg)


@pytest.mark.parametrize("case", VJP_CASES)
def test_forward_vjp(case):
    P = wc.problem(case)
    eng = engine_on(P)
    ybar = np.random.default_rng(11).standard_normal((P.N, P.cfg["O"])).astype(F32)
    nfbar, gs, out = eng.forward_vjp(P.nf, P.ef, ybar, want_out=True)
    rout, rg, rnf = orc.model_vjp(P.ps, P.cfg, P.nf, P.ef, P.s, P.r, lambda o: ybar.astype(np.float64))
    report("forward_vjp", case, out=rel_max(out, rout) / 1e-4)
    assert rel_max(out, rout) <= 1e-4
    assert nfbar.shape == (P.N, P.cfg["Fn"])
    check_pullback("forward_vjp", case, nfbar, rnf, gs, rg, P.cfg)


# ---- 6. the datapoint path -------------------------------------------------------------------------------------------------------
DATAPOINT_CASES = ["min", "cross64", "full64h3", "edge128"]
DT = F32(0.01)


class Mgn:
    """What init_train_step / build_graph read of the reference's GraphNetwork: the normalisers."""

    def __init__(self, n_norm, e_norm, o_norm):
        self.n_norm, self.e_norm, self.o_norm = n_norm, e_norm, o_norm


@pytest.mark.parametrize("case", DATAPOINT_CASES)
def test_datapoint_path(case):
    P = wc.problem(case)
    cfg, N, E = P.cfg, P.N, P.E
    Fn, Fe, O = cfg["Fn"], cfg["Fe"], cfg["O"]
    T = 3
    rng = np.random.default_rng(5)
    frames = (rng.standard_normal((T, N, O)) * rng.uniform(0.3, 1.5, O) + rng.uniform(-1, 1, O)).astype(F32)
    onehot = ra.one_hot(rng.integers(0, Fn - O, N), Fn - O) if Fn > O else None
    ef_raw = (rng.standard_normal((E, Fe)) * rng.uniform(0.1, 0.3, Fe) + rng.uniform(-0.3, 0.3, Fe)).astype(F32)
    noisy = rng.random(N) < 0.6
    stddev = rng.uniform(0.02, 0.05, O).astype(F32)
    mgn = Mgn({"velocity": ra.NormaliserOfflineMeanStd(rng.uniform(-1, 1, O), rng.uniform(0.5, 2, O)),
               "node_type": ra.NormaliserOfflineMinMax(0.0, 1.0)},
              ra.NormaliserOfflineMeanStd(rng.uniform(-0.3, 0.3, Fe), rng.uniform(0.1, 0.3, Fe)),
              {"velocity": ra.NormaliserOfflineMeanStd(rng.uniform(-3, 3, O), rng.uniform(30, 140, O))})
    vs, vsh = mgn.n_norm["velocity"].affine(O)
    ts, tsh = mgn.n_norm["node_type"].affine(Fn - O)
    node, edge, out = (np.concatenate([vs, ts]), np.concatenate([vsh, tsh])), mgn.e_norm.affine(Fe), mgn.o_norm["velocity"].inverse_affine(O)
    eng = engine_on(P)
    eng.set_norms(node=node, edge=edge, out=out)
    eng.set_trajectory(frames, dt=DT, node_type_onehot=onehot, ef_raw=ef_raw)
    eng.set_noise(stddev, noisy, seed=11)
    types = onehot if onehot is not None else np.zeros((N, 0), F32)
    worst = 0.0
    raws = []
    for t in range(T - 1):
        nf, ef, tq = eng.datapoint_export(t)
        rnf, ref_, d = eng.datapoint_export(t, normalised=False)
        assert rnf.shape == (N, Fn) and ref_.shape == (E, Fe) and d.shape == (N, O)
        cur = np.ascontiguousarray(rnf[:, :O])
        raws.append((cur, ref_, d))
        assert same_bits(cur[~noisy], frames[t][~noisy]) and np.all(cur[noisy] != frames[t][noisy])
        assert same_bits(rnf[:, O:], types) and same_bits(ref_, ef_raw)
        d_np = ((frames[t + 1] - cur) / DT).astype(F32)
        assert same_bits(d, d_np)
        assert same_bits(tq, ((d_np - out[1]) / out[0]).astype(F32))
        # the mirror: init_train_step on the noisy state the export shows
        data = {"velocity": np.stack([cur] * (T - 1)), "target|velocity": frames[1:]}
        g, mtq = ra.init_train_step_derivative(mgn, data, {"dt": float(DT)}, ["velocity"], ["velocity"], types, ef_raw, P.s, P.r, t)
        assert same_bits(tq, mtq)
        u_nf = affine_ulps(nf[:, :O], g.nf[:, :O], cur, node[0][:O], node[1][:O])
        u_ef = affine_ulps(ef, g.ef, ref_, edge[0], edge[1])
        worst = max(worst, u_nf / 2.0, u_ef / 2.0)
        assert u_nf <= 2.0 and u_ef <= 2.0, (u_nf, u_ef)
        assert same_bits(nf[:, O:], types)                            # (the reference's min-max normaliser of node_type over [0, 1])
        gs_a, loss_a = eng.step(nf, ef, tq, P.mask)
        gs_b, loss_b = eng.step_datapoint(t, P.mask)
        assert np.isfinite(loss_b) and np.abs(gs_b).max() > 0
        assert loss_a == loss_b and same_bits(gs_a, gs_b), (t, loss_a, loss_b)
    report("datapoint", case, affine_ulps=worst)
    # one accumulating step with all three online groups: the totals are mgn_feature_stats' of the raw rows, bit for bit
    eng.online_norms()
    eng.step_datapoint(0, P.mask, accumulate=True)
    for g_, (rows, raw) in enumerate(zip((N, E, N), raws[0])):
        s_, q_, count, calls = eng.norm_state(g_)
        ws, wq = eng.feature_stats(raw)
        assert same_bits(s_, ws) and same_bits(q_, wq), g_
        assert count == rows and calls == 1
        x64 = raw.astype(np.float64)
        assert np.allclose(ws, x64.sum(0), rtol=1e-12, atol=1e-9) and np.allclose(wq, (x64 * x64).sum(0), rtol=1e-12)   # ... which are the float64 sums


# ---- 7. solver training ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["out32", "cross64"])
def test_solver_grad(case):
    """Euler, three steps, inflow rows, loss_scale and the continuity term against the float64 discrete adjoint
    (tests/solver_adjoint_ref.py), at the tolerances of tests/test_gpu_solver_train.py"""
    P = wc.problem(case)
    N, O = P.N, P.cfg["O"]
    K = 3
    rng = np.random.default_rng(6)
    gt = (P.x[None] * (1.0 + 0.05 * rng.standard_normal((K + 1, N, O)))).astype(F32)
    frames = (P.x[None] * (1.0 + 0.2 * rng.standard_normal((K + 1, N, O)))).astype(F32)
    im = np.zeros(N, bool)
    im[[0, 7, 20, 41, N - 1]] = True
    ls = rng.uniform(0.5, 2.0, O).astype(F32)
    ct = (gt[-1] + 0.3 * rng.standard_normal((N, O))).astype(F32)
    kw = dict(val_mask=P.vm, inflow_mask=im.astype(np.uint8), inflow_data=frames, loss_scale=ls, cont_target=ct, cont_weight=0.05)
    eng = engine_on(P, norms=True)
    gs, loss, pred = eng.solver_grad(gt[0], P.onehot, P.ef, gt, 0.0, K * SDT, SDT, SDT, K + 1, want_pred=True, inflow_rule="reference",
                                     time_type=np.float32, **kw)
    oh = P.onehot if P.onehot is not None else np.zeros((N, 0), F32)
    norms = wc.oracle_norms(P)
    vm2 = P.vm[:, None].astype(np.float64)
    o_rhs = lambda x: orc.ode_rhs(P.ps, P.cfg, x, oh, P.ef, P.s, P.r, *norms, vm2)                       # noqa: E731
    o_vjp = lambda x, lam: orc.ode_vjp(P.ps, P.cfg, x, oh, P.ef, P.s, P.r, *norms, P.vm, lam)[:2]         # noqa: E731
    gs_o, loss_o, pred_o, _ = sar.euler_adjoint(o_rhs, o_vjp, gt[0], gt, 0.0, K * SDT, SDT, SDT, K + 1, inflow_rule="reference",
                                                time_type=np.float32, **kw)
    report("solver_grad", case, loss=abs(loss - loss_o) / abs(loss_o) / 1e-4, grad=rel_l2(gs, gs_o) / 5e-3, pred=rel_max(pred, pred_o) / 1e-4)
    assert abs(loss - loss_o) <= 1e-4 * abs(loss_o), (loss, loss_o)
    assert rel_l2(gs, gs_o) <= 5e-3, rel_l2(gs, gs_o)
    assert rel_max(pred, pred_o) <= 1e-4


# ---- 8. whole-array LayerNorm ----------------------------------------------------------------------------------------------------
@pytest.fixture
def whole_array_oracle():
    orc.LN_DIMS = "all"
    yield
    orc.LN_DIMS = "row"


@pytest.mark.parametrize("case", ["full32", "cross64"])
def test_whole_array_layernorm(whole_array_oracle, case):
    """ln_dims = MGN_LN_ALL runs its inference on the training kernels too: forward and step at the tolerances of
    tests/test_gpu_spec_variants.py"""
    P = wc.problem(case)
    eng = engine_on(P, ln_dims="all")
    err = rel_max(eng.forward(P.nf, P.ef), orc.forward(P.ps, P.cfg, P.nf, P.ef, P.s, P.r))
    g_ref, loss_ref = orc.step_grads(P.ps, P.cfg, P.nf, P.ef, P.s, P.r, P.target, P.mask)
    gs, loss = eng.step(P.nf, P.ef, P.target, P.mask)
    report("ln_all", case, out=err / TOL_15, loss=abs(loss - loss_ref) / (1e-5 * max(1.0, abs(loss_ref))), grad=rel_l2(gs, g_ref) / 2e-4)
    assert err <= TOL_15, err
    assert abs(loss - loss_ref) <= 1e-5 * max(1.0, abs(loss_ref)), (loss, loss_ref)
    assert rel_l2(gs, g_ref) <= 2e-4, rel_l2(gs, g_ref)


# ---- 9. two edge sets, the second of width L -------------------------------------------------------------------------------------
def test_two_edge_sets_with_the_second_of_width_L():
    cfg = dict(Fn=9, Fe=3, O=2, L=32, hidden_layers=2, mps=wc.MPS, Fe2=32)
    s, r, N = wc.mesh()
    rng = np.random.default_rng(9)
    s2, r2 = synth.random_graph(N, 40, 9)
    P = wc.Problem()
    P.cfg, P.s, P.r, P.N, P.E, P.ps = cfg, s, r, N, s.size, wc.params(cfg)
    P.nf, P.ef = rng.standard_normal((N, 9)).astype(F32), rng.standard_normal((s.size, 3)).astype(F32)
    ef2 = rng.standard_normal((s2.size, 32)).astype(F32)
    P.target = rng.standard_normal((N, 2)).astype(F32)
    P.mask = np.sort(rng.choice(N, N // 2, replace=False)).astype(np.int32)
    eng = engine_on(P)
    eng.set_edge_set(1, s2, r2)
    eng.set_edge_features(1, ef2)
    err = rel_max(eng.forward(P.nf, P.ef), orc.forward(P.ps, cfg, P.nf, P.ef, s, r, set2=(ef2, s2, r2)))
    report("two_sets", "Fe2=32", out=err / TOL_15)
    assert err <= TOL_15, err
    check_step(eng, P, "two_sets", "Fe2=32", set2=(ef2, s2, r2))


# ---- 10. two partitions ----------------------------------------------------------------------------------------------------------
def test_two_partitions():
    case = "cross64"
    P = wc.problem(case)
    cfg = P.cfg
    with GroupEngine(cfg["Fn"], cfg["Fe"], cfg["O"], cfg["L"], cfg["hidden_layers"], cfg["mps"], devices=[0, 0]) as g:
        g.set_params(P.ps)
        g.set_graph(P.s, P.r, P.N)
        assert all(g.rank_engine(k).n_own > 0 and g.rank_engine(k).n_halo > 0 for k in range(2))
        err = rel_max(g.forward(P.nf, P.ef), orc.forward(P.ps, cfg, P.nf, P.ef, P.s, P.r))
        report("two_partitions", case, out=err / TOL_15)
        assert err <= TOL_15, err
        check_step(g, P, "two_partitions", case)


# ---- 11. width sweep -------------------------------------------------------------------------------------------------------------
def draw_widths(seed):
    rng = np.random.default_rng(7000 + seed)
    L = int(rng.choice([32, 64, 128]))
    Fn, Fe = int(rng.integers(1, L + 1)), int(rng.integers(1, L + 1))
    O = int(rng.integers(1, min(Fn, 8) + 1))
    if seed % 4 == 3:
        O = Fn
    cfg = dict(Fn=Fn, Fe=Fe, O=O, L=L, hidden_layers=2, mps=int(rng.integers(1, 4)))
    N, E = int(rng.integers(1, 200)), int(rng.integers(0, 1500))
    s, r = synth.random_graph(N, E, seed)
    ps = orc.init_params(Fn, Fe, O, L, 2, cfg["mps"], seed=seed, ln_jitter=0.1)
    return rng, cfg, N, E, s, r, ps


@pytest.mark.parametrize("seed", range(12))
def test_width_sweep(seed):
    """forward and mgn_step on seeded draws of (L, Fn, Fe, O) with the assertions of
    tests/test_gpu_random_sweep.py::test_random_training_step (and its reasoning about ReLU kinks in fp32)"""
    rng, cfg, N, E, s, r, ps = draw_widths(seed)
    eng = engine_of(cfg)
    eng.set_params(ps)
    eng.set_graph(s, r, N)
    nf = rng.standard_normal((N, cfg["Fn"])).astype(F32)
    ef = rng.standard_normal((E, cfg["Fe"])).astype(F32)
    target = rng.standard_normal((N, cfg["O"])).astype(F32)
    mask = rng.choice(N, max(1, N // 2), replace=False).astype(np.int32)
    err = rel_max(eng.forward(nf, ef), orc.forward(ps, cfg, nf, ef, s, r))
    gs, loss = eng.step(nf, ef, target, mask)
    ref, ref_loss = orc.step_grads(ps, cfg, nf, ef, s, r, target, mask)
    err64 = np.linalg.norm(gs - ref) / np.linalg.norm(ref)
    print("WIDTHS sweep seed%d %s N=%d E=%d out=%.3g loss=%.3g grad=%.3g" % (seed, cfg, N, E, err / TOL_15,
                                                                            abs(loss - ref_loss) / (1e-5 * max(abs(ref_loss), 1e-6)), err64 / 2e-3))
    assert err <= TOL_15, (cfg, N, E, err)
    assert abs(loss - ref_loss) <= 1e-5 * max(abs(ref_loss), 1e-6), (cfg, N, E)
    if err64 > 2e-3:
        import torch_reference as tr
        g32, _ = tr.step(ps, cfg, nf, ef, s, r, target, mask, dtype=torch.float32, device="cuda")
        err32 = np.linalg.norm(gs - g32) / np.linalg.norm(ref)
        if err32 > 1e-4:
            assert err64 <= 5e-2, (cfg, N, E, err64)
            for trial in (1, 2):
                nf_j = (nf * (1.0 + 1e-4 * np.random.default_rng(trial).standard_normal(nf.shape))).astype(F32)
                gs_j, _ = eng.step(nf_j, ef, target, mask)
                ref_j, _ = orc.step_grads(ps, cfg, nf_j, ef, s, r, target, mask)
                assert np.linalg.norm(gs_j - ref_j) <= 2e-3 * np.linalg.norm(ref_j), (cfg, N, E, trial, err64, err32)
        else:
            assert err64 <= 5e-2, (cfg, N, E, err64, err32)


# ---- 12. refusals on a device handle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", wc.WIDE, ids=ids(wc.WIDE))
def test_training_is_refused_above_L_and_inference_goes_on(case):
    P = wc.problem(case)
    N, O = P.N, P.cfg["O"]
    eng = engine_on(P)
    gt = np.zeros((3, N, O), F32)
    calls = [lambda: eng.step(P.nf, P.ef, P.target, P.mask),
             lambda: eng.ode_vjp(P.x, P.onehot, P.ef, P.lam),
             lambda: eng.forward_vjp(P.nf, P.ef, P.lam),
             lambda: eng.solver_grad(P.x, P.onehot, P.ef, gt, 0.0, 0.02, 0.01, 0.01, 3),
             lambda: eng.set_trajectory(gt, dt=0.01, node_type_onehot=P.onehot, ef_raw=P.ef),
             lambda: eng.step_datapoint(0, P.mask)]
    for i, call in enumerate(calls):
        with pytest.raises(MgnError) as ei:
            call()
        assert ei.value.code == _capi.MGN_E_UNSUPPORTED, (i, str(ei.value))
        assert "L = %d" % P.cfg["L"] in str(ei.value)
    err = rel_max(eng.forward(P.nf, P.ef), orc.forward(P.ps, P.cfg, P.nf, P.ef, P.s, P.r))
    assert err <= TOL_15, err
