"""Training step (mgn_step == GraphNetCore.step!, reference src/strategies.jl:418-422) against the float64 hand-written
reverse-mode oracle (oracle/mgn_oracle.py step_grads, itself checked against finite differences on the CPU).
Run on the MI355X box with `-m gpu`."""
import numpy as np
import pytest
import torch   # before the engine's first HIP call (device-array test), or torch finds no GPU afterwards

import mgn_oracle as orc
import mgn_amd
from mgn_amd import synth
from train_checks import TOL_GRAD, TOL_LOSS, check_grads   # noqa: F401  (other test files take them from here)
from util import cfg_dict, engine_for, make_params, rel_max, small_mesh

pytestmark = pytest.mark.gpu


def problem(cfg, pos, s, r, seed=0, frac=0.6):
    N, E = pos.shape[0], s.size
    rng = np.random.default_rng(seed)
    nf = rng.standard_normal((N, cfg["Fn"])).astype(np.float32)
    ef = rng.standard_normal((E, cfg["Fe"])).astype(np.float32)
    target = rng.standard_normal((N, cfg["O"])).astype(np.float32)
    mask = np.sort(rng.choice(N, max(1, int(frac * N)), replace=False)).astype(np.int32)
    return nf, ef, target, mask


@pytest.mark.parametrize("L,mps", [(32, 1), (64, 2), (128, 3)])
def test_step_matches_oracle_small_mesh(L, mps):
    cfg = cfg_dict(L=L, mps=mps)
    pos, s, r = small_mesh(9, 7)
    ps = make_params(cfg)
    nf, ef, target, mask = problem(cfg, pos, s, r)
    eng = engine_for(cfg)
    eng.set_params(ps)
    eng.set_graph(s, r, pos.shape[0])
    gs, loss = eng.step(nf, ef, target, mask)
    ref, ref_loss = orc.step_grads(ps, cfg, nf, ef, s, r, target, mask)
    assert abs(loss - ref_loss) <= TOL_LOSS * abs(ref_loss), (loss, ref_loss)
    check_grads(gs, ref, cfg)
    gs2, loss2 = eng.step(nf, ef, target, mask)                     # deterministic: bitwise repeatable
    assert loss2 == loss and np.array_equal(gs, gs2)


def test_step_cyl_15_steps_one_based_mask():
    """cylinder_flow-shaped training datapoint (cfg-2 sized mesh, L = 128, 15 steps), mask 1-based as at the Julia
    boundary (src/MeshGraphNets.jl:352)."""
    cfg = cfg_dict(mps=15)
    pos, cells, node_type, vel = synth.mesh_cyl(1234, 700)
    s, r = synth.cells_to_edges(cells)
    ps = make_params(cfg, jitter=0.05)
    nf, ef, target, _ = problem(cfg, pos, s, r, seed=3)
    mask0 = np.nonzero(np.isin(node_type, [0, 5]))[0].astype(np.int32)      # types_updated, like val_mask
    eng = engine_for(cfg)
    eng.set_params(ps)
    eng.set_graph(s, r, pos.shape[0])
    gs, loss = eng.step(nf, ef, target, mask0 + 1, mask_index_base=1)
    ref, ref_loss = orc.step_grads(ps, cfg, nf, ef, s, r, target, mask0)
    assert abs(loss - ref_loss) <= TOL_LOSS * abs(ref_loss), (loss, ref_loss)
    check_grads(gs, ref, cfg)
    # the forward inside step! is the model: same output as mgn_forward
    out = eng.forward(nf, ef)
    assert abs(float(orc.mse_reduce(target, out)[mask0].mean()) - loss) <= 1e-4 * abs(loss)


@pytest.mark.parametrize("factored", [None, "1"])
@pytest.mark.parametrize("N,E,seed,L", [(1, 0, 0, 128), (33, 31, 2, 128), (40, 700, 3, 128), (70, 2049, 5, 128), (233, 106, 7, 64), (97, 40, 8, 32)])
def test_step_ragged_graphs(N, E, seed, L, factored, monkeypatch):
    """isolated nodes, self loops, duplicate edges, heavy receivers, no edges at all, fewer edges than nodes; with the
    un-factored and (forced: these sizes would not pick it) the factored first layer of the edge MLPs"""
    if factored:
        monkeypatch.setenv("MGN_TRAIN_FACTORED", factored)
    cfg = cfg_dict(L=L, mps=2)
    s, r = synth.random_graph(N, E, seed)
    ps = make_params(cfg)
    rng = np.random.default_rng(seed)
    nf = rng.standard_normal((N, 9)).astype(np.float32)
    ef = rng.standard_normal((E, 3)).astype(np.float32)
    target = rng.standard_normal((N, 2)).astype(np.float32)
    mask = np.arange(0, N, 2, dtype=np.int32)
    eng = engine_for(cfg)
    eng.set_params(ps)
    eng.set_graph(s, r, N)
    gs, loss = eng.step(nf, ef, target, mask)
    ref, ref_loss = orc.step_grads(ps, cfg, nf, ef, s, r, target, mask)
    assert abs(loss - ref_loss) <= TOL_LOSS * max(abs(ref_loss), 1e-6)
    check_grads(gs, ref, cfg, tol=TOL_GRAD if not factored else 2e-3)   # factored: another summation order at the ReLU kinks


def test_step_descends_and_tracks_new_params():
    """A few plain gradient-descent updates through set_params / step: the loss falls, and the gradients follow the
    parameters that were uploaded last (the training-order weight copy is rebuilt)."""
    cfg = cfg_dict(L=64, mps=2)
    pos, s, r = small_mesh(8, 6)
    ps = make_params(cfg).astype(np.float32)
    nf, ef, target, mask = problem(cfg, pos, s, r, seed=9)
    eng = engine_for(cfg)
    eng.set_graph(s, r, pos.shape[0])
    losses = []
    for it in range(6):
        eng.set_params(ps)
        gs, loss = eng.step(nf, ef, target, mask)
        losses.append(loss)
        if it == 3:
            ref, _ = orc.step_grads(ps, cfg, nf, ef, s, r, target, mask)
            check_grads(gs, ref, cfg)
        ps = ps - 0.01 * gs
    assert losses[-1] < losses[0], losses


def test_step_argument_errors():
    import mgn_amd
    cfg = cfg_dict(L=32, mps=1)
    pos, s, r = small_mesh(5, 4)
    N = pos.shape[0]
    eng = engine_for(cfg)
    eng.set_params(make_params(cfg))
    eng.set_graph(s, r, N)
    nf, ef, target, mask = problem(cfg, pos, s, r)
    with pytest.raises(mgn_amd.MgnError) as ei:
        eng.step(nf, ef, target, np.array([N], np.int32))            # out of range (0-based)
    assert ei.value.code == -1
    with pytest.raises(mgn_amd.MgnError) as ei:
        eng.step(nf, ef, target, np.array([0], np.int32), mask_index_base=1)
    assert ei.value.code == -1
    with pytest.raises(mgn_amd.MgnError) as ei:
        eng.step(nf, ef, target, np.zeros(0, np.int32))
    assert ei.value.code == -1
    bf = mgn_amd.Engine(9, 3, 2, 128, 2, 1, dtype="bf16")
    bf.set_params(make_params(cfg_dict(mps=1)))
    bf.set_graph(s, r, N)
    with pytest.raises(mgn_amd.MgnError) as ei:
        bf.step(nf, ef, target, mask)
    assert ei.value.code == -3


def test_ode_vjp_matches_oracle_and_ode_step():
    """mgn_ode_vjp: lambda^T df/dx, lambda^T df/dps of the RHS the solver-based strategies differentiate
    (src/strategies.jl:175-196), with frozen normalisers and val_mask like mgn_ode_step."""
    cfg = cfg_dict(mps=3)
    pos, cells, node_type, vel = synth.mesh_cyl(1234, 300)
    s, r = synth.cells_to_edges(cells)
    N, E = pos.shape[0], s.size
    ps = make_params(cfg)
    rng = np.random.default_rng(4)
    onehot = orc.one_hot(node_type, 7, 0).astype(np.float32)
    ef_raw = orc.edge_features(pos, s, r).astype(np.float32)
    x = vel.astype(np.float32)
    lam = rng.standard_normal((N, 2)).astype(np.float32)
    n_norm = orc.NormMeanStd(np.array([1.0, 0.1]), np.array([0.4, 0.2]))
    t_norm = orc.NormMinMax(0.0, 1.0)
    e_norm = orc.NormMeanStd(ef_raw.mean(0), ef_raw.std(0))
    o_norm = orc.NormMeanStd(np.array([0.01, -0.02]), np.array([0.5, 0.4]))
    vm = np.isin(node_type, [0, 5]).astype(np.float32)
    ns, nsh = n_norm.affine(2)
    ts, tsh = t_norm.affine(7)
    es, esh = e_norm.affine(3)
    eng = engine_for(cfg)
    eng.set_params(ps)
    eng.set_graph(s, r, N)
    eng.set_norms(node=(np.concatenate([ns, ts]), np.concatenate([nsh, tsh])), edge=(es, esh), out=(o_norm.std, o_norm.mean))
    xbar, gs, dxdt = eng.ode_vjp(x, onehot, ef_raw, lam, val_mask=vm, want_dxdt=True)
    rx, rg, rf = orc.ode_vjp(ps, cfg, x, onehot, ef_raw, s, r, n_norm, t_norm, e_norm, o_norm, vm, lam)
    assert rel_max(dxdt, rf) <= 1e-4
    assert np.array_equal(dxdt, eng.ode_step(x, onehot, ef_raw, vm)) or rel_max(dxdt, eng.ode_step(x, onehot, ef_raw, vm)) <= 1e-5
    # ReLU kinks: with ~1e6 hidden units per evaluation about one pre-activation lies within fp32 rounding of zero, and
    # the engine's summation order may put it on the other side than the oracle's -- the derivative through that ONE
    # unit then differs (seen here: one edge-MLP unit, both end nodes of that edge off by 3 %, everything else 1e-6).
    # Hence a robust criterion: all but 2 % of the rows within TOL_GRAD, and a small relative L2 error overall.
    row_err = np.abs(xbar - rx).max(1) / np.abs(rx).max()
    assert np.quantile(row_err, 0.98) <= TOL_GRAD, np.quantile(row_err, 0.98)
    assert np.linalg.norm(xbar - rx) <= 5e-3 * np.linalg.norm(rx)
    assert np.linalg.norm(gs - rg) <= 5e-3 * np.linalg.norm(rg)
    check_grads(gs, rg, cfg, tol=2e-2)
    # coarse self-consistency with the engine's own RHS (sign and scale): <lambda, f(x + eps d) - f(x - eps d)> / 2 eps vs
    # <xbar, d>.  f is strongly nonlinear (the float64 oracle needs eps <= 1e-4 for 1 %) and fp32 forbids a smaller eps.
    d = rng.standard_normal((N, 2)).astype(np.float32)
    eps = 1e-3
    fd = float((lam.astype(np.float64) * (eng.ode_step(x + eps * d, onehot, ef_raw, vm).astype(np.float64)
                                          - eng.ode_step(x - eps * d, onehot, ef_raw, vm))).sum() / (2 * eps))
    an = float((xbar.astype(np.float64) * d).sum())
    assert abs(fd - an) <= 0.2 * abs(an), (fd, an)


def test_forward_vjp_is_the_pullback_of_the_model_call():
    """mgn_forward_vjp: the pullback of `output, st = mgn.model(graph, ps, mgn.st)` (reference src/solve.jl:200) -- what the Julia shim's
    ChainRulesCore.rrule hands to Zygote when it differentiates ode_func_train as written (src/strategies.jl:183-195): for a cotangent
    ybar of the output, ybar^T d out / d nf (all Fn columns) and ybar^T d out / d ps, against the oracle's reverse mode; composing it
    with the Julia-side pieces (normalisers, inverse_data, val_mask) by hand reproduces mgn_ode_vjp."""
    cfg = cfg_dict(mps=3)
    pos, cells, node_type, vel = synth.mesh_cyl(1234, 300)
    s, r = synth.cells_to_edges(cells)
    N, E = pos.shape[0], s.size
    ps = make_params(cfg)
    rng = np.random.default_rng(11)
    nf = rng.standard_normal((N, 9)).astype(np.float32)
    ef = rng.standard_normal((E, 3)).astype(np.float32)
    ybar = rng.standard_normal((N, 2)).astype(np.float32)
    eng = engine_for(cfg)
    eng.set_params(ps)
    eng.set_graph(s, r, N)
    nfbar, gs, out = eng.forward_vjp(nf, ef, ybar, want_out=True)
    rout, rg, rnf = orc.model_vjp(ps, cfg, nf, ef, s, r, lambda o: ybar.astype(np.float64))
    assert rel_max(out, rout) <= 1e-4
    assert rel_max(out, eng.forward(nf, ef)) <= 1e-5
    row_err = np.abs(nfbar - rnf).max(1) / np.abs(rnf).max()
    assert np.quantile(row_err, 0.98) <= TOL_GRAD, np.quantile(row_err, 0.98)
    assert np.linalg.norm(nfbar - rnf) <= 5e-3 * np.linalg.norm(rnf)
    assert np.linalg.norm(gs - rg) <= 5e-3 * np.linalg.norm(rg)
    check_grads(gs, rg, cfg, tol=2e-2)
    # the chain rule around it, as Zygote would apply it to ode_step: nf = [n_norm(x); n_norm(onehot)], dx/dt = (out * os + osh) .* vm
    onehot = orc.one_hot(node_type, 7, 0).astype(np.float32)
    ef_raw = orc.edge_features(pos, s, r).astype(np.float32)
    n_scale, n_shift = np.array([2.5, 5.0], np.float32), np.array([-2.5, -0.5], np.float32)
    e_scale, e_shift = (1 / ef_raw.std(0)).astype(np.float32), (-ef_raw.mean(0) / ef_raw.std(0)).astype(np.float32)
    o_scale, o_shift = np.array([0.5, 0.4], np.float32), np.array([0.01, -0.02], np.float32)
    vm = np.isin(node_type, [0, 5]).astype(np.float32)
    x = vel.astype(np.float32)
    lam = rng.standard_normal((N, 2)).astype(np.float32)
    eng.set_norms(node=(np.concatenate([n_scale, np.ones(7, np.float32)]), np.concatenate([n_shift, np.zeros(7, np.float32)])),
                  edge=(e_scale, e_shift), out=(o_scale, o_shift))
    xbar, gs_f, _ = eng.ode_vjp(x, onehot, ef_raw, lam, val_mask=vm)
    nf2 = np.concatenate([x * n_scale + n_shift, onehot], 1)
    nfbar2, gs2, _ = eng.forward_vjp(nf2, ef_raw * e_scale + e_shift, lam * vm[:, None] * o_scale)
    assert np.linalg.norm(nfbar2[:, :2] * n_scale - xbar) <= 1e-4 * np.linalg.norm(xbar)
    assert np.linalg.norm(gs2 - gs_f) <= 1e-4 * np.linalg.norm(gs_f)
    with pytest.raises(mgn_amd.MgnError):                                  # null arguments: MGN_E_ARG, like the reference's ArgumentError
        eng._chk(eng.lib.mgn_forward_vjp(eng.h, None, None, None, None, None, None, 0))


def test_recompute_mode_gives_the_same_gradients(monkeypatch):
    """Large meshes keep H1 / H2 / Y of as many processor steps as memory holds and recompute the others in the reverse pass from their
    kept inputs (MGN_TRAIN_RECOMPUTE forces all or none, MGN_TRAIN_KEEP_STEPS the count): same forward arithmetic, so loss and
    gradients are bitwise equal in every split."""
    import ctypes as C
    cfg = cfg_dict(L=128, mps=3)
    pos, s, r = small_mesh(12, 9)
    ps = make_params(cfg)
    nf, ef, target, mask = problem(cfg, pos, s, r, seed=21)
    res = []
    for env, want in ((("MGN_TRAIN_RECOMPUTE", "0"), 3), (("MGN_TRAIN_RECOMPUTE", "1"), 0), (("MGN_TRAIN_KEEP_STEPS", "1"), 1),
                      (("MGN_TRAIN_KEEP_STEPS", "2"), 2)):
        monkeypatch.delenv("MGN_TRAIN_RECOMPUTE", raising=False)
        monkeypatch.delenv("MGN_TRAIN_KEEP_STEPS", raising=False)
        monkeypatch.setenv(*env)
        eng = engine_for(cfg)
        eng.set_params(ps)
        eng.set_graph(s, r, pos.shape[0])
        res.append(eng.step(nf, ef, target, mask))
        eng.lib.mgn_debug_train_keep_steps.argtypes = [C.c_void_p]
        assert eng.lib.mgn_debug_train_keep_steps(eng.h) == want
    for other in res[1:]:
        assert res[0][1] == other[1] and np.array_equal(res[0][0], other[0])
    ref, _ = orc.step_grads(ps, cfg, nf, ef, s, r, target, mask)
    check_grads(res[1][0], ref, cfg)


def test_arena_allocation_is_retried_with_fewer_stored_steps(monkeypatch):
    """The arena of a large mesh takes what the device reports free; a request that is refused all the same (another process was faster)
    is retried with half the stored steps, down to none (MGN_TRAIN_TEST_FAIL_ALLOCS counts requests as refused): same bits, and a
    clean MGN_E_OOM when even the arena without stored steps is refused."""
    import ctypes as C
    cfg = cfg_dict(L=128, mps=3)
    pos, s, r = small_mesh(12, 9)
    ps = make_params(cfg)
    nf, ef, target, mask = problem(cfg, pos, s, r, seed=21)
    res = []
    for fails, want in ((0, 3), (1, 1), (2, 0)):
        monkeypatch.setenv("MGN_TRAIN_TEST_FAIL_ALLOCS", str(fails))
        eng = engine_for(cfg)
        eng.set_params(ps)
        eng.set_graph(s, r, pos.shape[0])
        res.append(eng.step(nf, ef, target, mask))
        eng.lib.mgn_debug_train_keep_steps.argtypes = [C.c_void_p]
        assert eng.lib.mgn_debug_train_keep_steps(eng.h) == want
    for other in res[1:]:
        assert res[0][1] == other[1] and np.array_equal(res[0][0], other[0])
    monkeypatch.setenv("MGN_TRAIN_TEST_FAIL_ALLOCS", "3")
    eng = engine_for(cfg)
    eng.set_params(ps)
    eng.set_graph(s, r, pos.shape[0])
    with pytest.raises(mgn_amd.MgnError):
        eng.step(nf, ef, target, mask)


def test_step_device_arrays_and_graph_replay():
    """nf / ef / target / grads may live on the device (hipMemcpyDefault, include/mgn_hip.h): same bits as the host call.  Four
    calls in a row take the small-mesh path through its three stages -- eager, hipGraph capture, replay (forward and backward
    sequences, the weight gradients on the second stream) -- and have to agree bitwise; new inputs must show through a replay."""
    import torch
    cfg = cfg_dict(L=128, mps=3)
    pos, s, r = small_mesh(14, 11)
    ps = make_params(cfg)
    nf, ef, target, mask = problem(cfg, pos, s, r, seed=33)
    eng = engine_for(cfg)
    eng.set_params(ps)
    eng.set_graph(s, r, pos.shape[0])
    host = [eng.step(nf, ef, target, mask) for _ in range(4)]
    for g, l in host[1:]:
        assert l == host[0][1] and np.array_equal(g, host[0][0])
    d = lambda a: torch.from_numpy(a).cuda()
    out = torch.zeros(eng.param_count, device="cuda")
    g_dev, l_dev = eng.step(d(nf), d(ef), d(target), mask, out=out)
    assert g_dev is out and l_dev == host[0][1] and np.array_equal(out.cpu().numpy(), host[0][0])
    buf = np.full(eng.param_count, np.nan, np.float32)
    eng.step(nf, ef, target, mask, out=buf)
    assert np.array_equal(buf, host[0][0])
    nf2 = nf + 0.25
    g2, l2 = eng.step(nf2, ef, target, mask)                 # replayed graphs, new inputs
    ref, rl = orc.step_grads(ps, cfg, nf2, ef, s, r, target, mask)
    assert abs(l2 - rl) <= TOL_LOSS * abs(rl)
    check_grads(g2, ref, cfg)
    with pytest.raises(ValueError):
        eng.step(nf, ef, target, mask, out=np.zeros(eng.param_count + 1, np.float32))


def test_graph_slots_shared_across_entry_points():
    """mgn_step, mgn_ode_vjp and mgn_forward_vjp interleaved on one handle: the forward sequence (graph slot 0) is every entry's, the step's
    reverse pass has slot 1 and the two VJPs share slot 2.  Four rounds take each slot through eager run, capture and replay with another
    entry's launches in between; every output has to be bitwise the same in all rounds and equal to what a fresh handle returns on its
    first (eager) call of that entry alone.  New inputs must show through the replays: the step against the oracle."""
    cfg = cfg_dict(L=128, mps=3)
    pos, s, r = small_mesh(14, 11)
    N = pos.shape[0]
    ps = make_params(cfg)
    nf, ef, target, mask = problem(cfg, pos, s, r, seed=41)
    rng = np.random.default_rng(42)
    onehot = orc.one_hot(rng.integers(0, 7, N), 7, 0).astype(np.float32)
    ef_raw = orc.edge_features(pos, s, r).astype(np.float32)
    x = rng.standard_normal((N, 2)).astype(np.float32)
    lam = rng.standard_normal((N, 2)).astype(np.float32)
    ybar = rng.standard_normal((N, 2)).astype(np.float32)
    vm = (rng.random(N) < 0.7).astype(np.float32)
    ns, nsh = orc.NormMeanStd(np.array([1.0, 0.1]), np.array([0.4, 0.2])).affine(2)
    ts, tsh = orc.NormMinMax(0.0, 1.0).affine(7)
    es, esh = orc.NormMeanStd(ef_raw.mean(0), ef_raw.std(0)).affine(3)

    def engine():
        eng = engine_for(cfg)
        eng.set_params(ps)
        eng.set_graph(s, r, N)
        eng.set_norms(node=(np.concatenate([ns, ts]), np.concatenate([nsh, tsh])), edge=(es, esh), out=(np.array([0.5, 0.4]), np.array([0.01, -0.02])))
        return eng

    entries = {
        "step": lambda e, d=0.0: e.step(nf + d, ef, target, mask),
        "ode_vjp": lambda e, d=0.0: e.ode_vjp(x + d, onehot, ef_raw, lam, val_mask=vm, want_dxdt=True),
        "forward_vjp": lambda e, d=0.0: e.forward_vjp(nf + d, ef, ybar, want_out=True),
    }
    same = lambda a, b: all(np.array_equal(np.asarray(u), np.asarray(v)) for u, v in zip(a, b))
    eng = engine()
    rounds = [{k: f(eng) for k, f in entries.items()} for _ in range(4)]
    for k, f in entries.items():
        for rd in rounds[1:]:
            assert same(rd[k], rounds[0][k]), k
            assert k != "step" or rd[k][1] == rounds[0][k][1]
        assert same(f(engine()), rounds[0][k]), k                  # a fresh handle's first call of this entry alone
    fifth = {k: f(eng, np.float32(0.25)) for k, f in entries.items()}     # replayed graphs, new inputs
    for k in entries:
        assert not any(np.array_equal(np.asarray(u), np.asarray(v)) for u, v in zip(fifth[k], rounds[0][k])), k
    ref, rl = orc.step_grads(ps, cfg, nf + np.float32(0.25), ef, s, r, target, mask)
    assert abs(fifth["step"][1] - rl) <= TOL_LOSS * abs(rl)
    check_grads(fifth["step"][0], ref, cfg)


def test_step_factored_first_layer_above_the_cooperative_range(monkeypatch):
    """Above 2048 edge tiles the edge MLPs run with the factored first layer (P = v W1s, Q = v W1r per node; backward and
    weight gradients through the summed rows of GZ1): against the float64 oracle and against the un-factored kernels on
    the same inputs.  With ~2e7 hidden units per evaluation a few pre-activations lie within fp32 rounding of the ReLU kink
    and the two summation orders may decide them differently (one column of one weight gradient moves by ~1e-3 then):
    relative L2 over the whole gradient, not a per-entry bound."""
    cfg = cfg_dict(L=128, mps=2)
    pos, s, r = synth.mesh_1m(7, 110, 110)
    assert (s.size + 31) // 32 > 2048
    ps = make_params(cfg)
    nf, ef, target, mask = problem(cfg, pos, s, r, seed=5, frac=0.3)
    res = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("MGN_TRAIN_FACTORED", mode)
        eng = engine_for(cfg)
        eng.set_params(ps)
        eng.set_graph(s, r, pos.shape[0])
        res[mode] = eng.step(nf, ef, target, mask)
        g2, l2 = eng.step(nf, ef, target, mask)
        assert l2 == res[mode][1] and np.array_equal(g2, res[mode][0])          # deterministic
    monkeypatch.delenv("MGN_TRAIN_FACTORED")
    eng = engine_for(cfg)
    eng.set_params(ps)
    eng.set_graph(s, r, pos.shape[0])
    auto = eng.step(nf, ef, target, mask)
    assert auto[1] == res["1"][1] and np.array_equal(auto[0], res["1"][0])       # the size rule picks the factored path here
    ref, ref_loss = orc.step_grads(ps, cfg, nf, ef, s, r, target, mask)
    for mode in ("1", "0"):
        gs, loss = res[mode]
        assert abs(loss - ref_loss) <= TOL_LOSS * abs(ref_loss), (mode, loss, ref_loss)
        assert np.linalg.norm(gs - ref) <= 1e-3 * np.linalg.norm(ref), (mode, np.linalg.norm(gs - ref) / np.linalg.norm(ref))
    assert np.linalg.norm(res["1"][0] - res["0"][0]) <= 1e-3 * np.linalg.norm(ref)


def test_step_streaming_kernels_on_a_graph_with_hubs_and_isolated_nodes():
    """The streaming kernels' own aggregation (round 6: a segmented scan inside the forward's edge launch, carry rows for runs that cross
    32-edge tiles, a fix-up pass) and the LayerNorm job of the weight-gradient launch on a graph that is not a mesh: one node receives
    300 edges (its run covers whole tiles), one in ten receives none, the rest 0-30; 2 300 edge tiles (above the cooperative range)."""
    cfg = cfg_dict(L=128, mps=2)
    rng = np.random.default_rng(31)
    N, E = 9000, 73600
    deg = rng.integers(0, 31, N)
    deg[rng.choice(N, N // 10, replace=False)] = 0
    deg[17] = 300
    deg[N - 1] = 0
    r = np.repeat(np.arange(N), deg)
    r = np.concatenate([r, rng.integers(0, N, max(0, E - r.size))])[:E].astype(np.int32)
    s = rng.integers(0, N, E).astype(np.int32)
    perm = rng.permutation(E)                              # the caller's edge order is arbitrary
    s, r = s[perm], r[perm]
    assert (E + 31) // 32 > 2048 and np.bincount(r, minlength=N).max() >= 300 and (np.bincount(r, minlength=N) == 0).sum() > 100
    pos = rng.random((N, 2)).astype(np.float32)
    ps = make_params(cfg)
    nf, ef, target, mask = problem(cfg, pos, s, r, seed=6, frac=0.3)
    eng = engine_for(cfg)
    eng.set_params(ps)
    eng.set_graph(s, r, N)
    gs, loss = eng.step(nf, ef, target, mask)
    g2, l2 = eng.step(nf, ef, target, mask)
    assert l2 == loss and np.array_equal(g2, gs)
    ref, ref_loss = orc.step_grads(ps, cfg, nf, ef, s, r, target, mask)
    assert abs(loss - ref_loss) <= TOL_LOSS * abs(ref_loss), (loss, ref_loss)
    assert np.linalg.norm(gs - ref) <= 1e-3 * np.linalg.norm(ref), np.linalg.norm(gs - ref) / np.linalg.norm(ref)


def test_stored_and_recomputed_steps_agree_beyond_32_bit_offsets(monkeypatch):
    """The arena of a 250 000-node mesh with 15 processor steps holds 40 GB when every step's activations are stored (offsets beyond
    2^32 bytes): all stored, seven of fifteen stored and none stored give the same bits; the size rule itself keeps them all (free memory
    decides, and the part has it)."""
    import ctypes as C
    cfg = cfg_dict(L=128, mps=15)
    pos, s, r = synth.mesh_1m(11, 500, 500)
    ps = make_params(cfg)
    nf, ef, target, mask = problem(cfg, pos, s, r, seed=8, frac=0.25)
    res = []
    for keep in ("15", "7", "0", None):
        if keep is None:
            monkeypatch.delenv("MGN_TRAIN_KEEP_STEPS", raising=False)
        else:
            monkeypatch.setenv("MGN_TRAIN_KEEP_STEPS", keep)
        eng = engine_for(cfg)
        eng.set_params(ps)
        eng.set_graph(s, r, pos.shape[0])
        res.append(eng.step(nf, ef, target, mask))
        eng.lib.mgn_debug_train_keep_steps.argtypes = [C.c_void_p]
        assert eng.lib.mgn_debug_train_keep_steps(eng.h) == (15 if keep is None else int(keep))
        eng.close()
    assert np.isfinite(res[0][0]).all() and np.isfinite(res[0][1])
    for other in res[1:]:
        assert other[1] == res[0][1] and np.array_equal(other[0], res[0][0])


def test_solver_training_euler_discrete_adjoint():
    """train_step(::SolverTraining) with fixed-step Euler (reference src/strategies.jl:175-196, 257-292) through
    mgn_ode_step + mgn_ode_vjp, against the same discrete adjoint driven by the float64 oracle, and against a central
    difference of the oracle's own loss in one parameter direction."""
    from mgn_amd import reference_api as ra
    cfg = cfg_dict(L=64, mps=2)
    pos, cells, node_type, vel = synth.mesh_cyl(1234, 150)
    s, r = synth.cells_to_edges(cells)
    N = pos.shape[0]
    ps = make_params(cfg).astype(np.float32)
    rng = np.random.default_rng(6)
    onehot = orc.one_hot(node_type, 7, 0).astype(np.float32)
    ef_raw = orc.edge_features(pos, s, r).astype(np.float32)
    K, dt = 4, 0.01
    gt = (vel[None] * (1.0 + 0.05 * rng.standard_normal((K + 1, N, 2)))).astype(np.float32)
    n_norm = orc.NormMeanStd(np.array([1.0, 0.1]), np.array([0.4, 0.2]))
    t_norm = orc.NormMinMax(0.0, 1.0)
    e_norm = orc.NormMeanStd(ef_raw.mean(0), ef_raw.std(0))
    o_norm = orc.NormMeanStd(np.array([0.01, -0.02]), np.array([5.0, 4.0]))
    vm = np.isin(node_type, [0, 5]).astype(np.float32)
    ns, nsh = n_norm.affine(2)
    ts, tsh = t_norm.affine(7)
    es, esh = e_norm.affine(3)
    eng = engine_for(cfg)
    eng.set_params(ps)
    eng.set_graph(s, r, N)
    eng.set_norms(node=(np.concatenate([ns, ts]), np.concatenate([nsh, tsh])), edge=(es, esh), out=(o_norm.std, o_norm.mean))

    gs, loss, xs = ra.solver_training_euler(lambda x: eng.ode_step(x, onehot, ef_raw, vm),
                                            lambda x, lam: eng.ode_vjp(x, onehot, ef_raw, lam, val_mask=vm)[:2], gt[0], gt, dt, vm, ns)

    def o_rhs(p):
        return lambda x: orc.ode_rhs(p, cfg, x, onehot, ef_raw, s, r, n_norm, t_norm, e_norm, o_norm, vm[:, None].astype(np.float64))

    def o_vjp(x, lam):
        return orc.ode_vjp(ps, cfg, x, onehot, ef_raw, s, r, n_norm, t_norm, e_norm, o_norm, vm, lam)[:2]

    gs_o, loss_o, xs_o = ra.solver_training_euler(o_rhs(ps), o_vjp, gt[0], gt, dt, vm, ns)
    assert abs(loss - loss_o) <= 1e-4 * abs(loss_o), (loss, loss_o)
    assert rel_max(xs[-1], xs_o[-1]) <= 1e-4
    assert np.linalg.norm(gs - gs_o) <= 5e-3 * np.linalg.norm(gs_o), np.linalg.norm(gs - gs_o) / np.linalg.norm(gs_o)
    # the adjoint really is the gradient of that loss: directional central difference on the float64 oracle
    d = rng.standard_normal(ps.size)
    d /= np.linalg.norm(d)
    eps = 1e-4

    def loss_at(p):
        return ra.solver_training_euler(o_rhs(p), lambda x, lam: (np.zeros_like(x), np.zeros(ps.size)), gt[0], gt, dt, vm, ns)[1]

    fd = (loss_at(ps.astype(np.float64) + eps * d) - loss_at(ps.astype(np.float64) - eps * d)) / (2 * eps)
    assert abs(fd - float(gs_o @ d)) <= 1e-3 * max(abs(fd), 1e-9), (fd, float(gs_o @ d))
