"""Derivative-training loop on P edge-cut partitions that share ONE GPU (GroupEngine): 50 iterations, new parameters before every step.
(a) GroupEngine.step on host arrays -- every rank stages the mesh's nf / ef / target from the host and gathers its rows, per step
(b) GroupEngine.step_datapoint on the trajectory resident on the ranks -- no input crosses PCIe per step
on the cylinder-sized mesh and on a 354 x 354 grid (125 316 nodes), P = 2 and P = 4.  Alternating blocks, three rounds after a warm-up
round; ms per iteration, host clock around calls that end in a stream synchronise.  Ranks that share a GPU serialise: the figures say
what staging costs a step, not how partitions scale.  Bytes are computed from the shapes.

    python3 tools/group_datapoint_timing.py [out.json]"""
import json, os, sys, time
import numpy as np
import torch  # noqa: F401  (before the engine's first HIP call)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "oracle"))
import mgn_amd
import mgn_oracle as orc

L, MPS, FN, FE, O = 128, 15, 9, 3, 2
ITERS, ROUNDS, T = 50, 3, 51
ps0 = orc.init_params(FN, FE, O, L, 2, MPS, seed=1234, ln_jitter=0.1).astype(np.float32)


def meshes():
    pos, cells, _, _ = mgn_amd.synth.mesh_cyl(1234, 2000)
    yield "M-cyl", pos, mgn_amd.synth.cells_to_edges(cells)
    pos, cells = mgn_amd.synth.grid_mesh(354, 354, 1)
    yield "grid-354x354", pos, mgn_amd.synth.cells_to_edges(cells)


def run(name, pos, s, r, P):
    N, E = pos.shape[0], s.size
    rng = np.random.default_rng(0)
    frames = (0.01 * np.cumsum(rng.standard_normal((T, N, O)), 0)).astype(np.float32)
    onehot = orc.one_hot(rng.integers(0, FN - O, N), FN - O, 0).astype(np.float32)
    rel = pos[s] - pos[r]
    ef_raw = np.concatenate([rel, np.linalg.norm(rel, axis=1, keepdims=True)], 1).astype(np.float32)[:, :FE]
    mask = np.sort(rng.choice(N, N // 2, replace=False)).astype(np.int32)
    d = (frames[1:] - frames[:-1]) / np.float32(0.01)
    one, zero = np.ones(FN - O, np.float32), np.zeros(FN - O, np.float32)
    sd = frames.std((0, 1))
    norms = dict(node=(np.concatenate([1 / sd, one]), np.concatenate([-frames.mean((0, 1)) / sd, zero])),
                 edge=(1 / ef_raw.std(0), -ef_raw.mean(0) / ef_raw.std(0)), out=(d.std((0, 1)), d.mean((0, 1))))
    ps = ps0.copy()
    gs = np.zeros(ps.size, np.float32)
    with mgn_amd.GroupEngine(FN, FE, O, L, 2, MPS, devices=[0] * P) as g:
        g.set_params(ps)
        g.set_norms(**norms)
        g.set_graph(s, r, N, mesh_pos=pos)
        g.set_trajectory(frames, dt=0.01, node_type_onehot=onehot, ef_raw=ef_raw)
        own = [g.rank_engine(k).n_own for k in range(P)]
        pre = [g.datapoint_export(t) for t in range(ITERS)]

        def new_params():
            nonlocal ps
            ps = ps * np.float32(1.00001)
            g.set_params(ps)

        def block_step():
            for t in range(ITERS):
                new_params()
                g.step(*pre[t], mask, out=gs)

        def block_datapoint():
            for t in range(ITERS):
                new_params()
                g.step_datapoint(t, mask, out=gs)

        res = {"a_group_step_host_arrays": [], "b_group_step_datapoint": []}
        for rnd in range(ROUNDS + 1):              # round 0 warms both paths
            for key, fn in (("a_group_step_host_arrays", block_step), ("b_group_step_datapoint", block_datapoint)):
                g.synchronize()
                t0 = time.perf_counter()
                fn()
                g.synchronize()
                if rnd:
                    res[key].append((time.perf_counter() - t0) / ITERS * 1e3)
        ga, la = g.step(*pre[3], mask)
        ga = np.array(ga)
        gb, lb = g.step_datapoint(3, mask)
        same = bool(la == lb and np.array_equal(ga, gb))
    params_b = int(ps.size) * 4
    return dict(mesh=name, N=int(N), E=int(E), P=P, n_own=own, same_bits=same,
                ms_per_iteration={k: {"median": float(np.median(v)), "all": [round(x, 3) for x in v]} for k, v in res.items()},
                h2d_bytes_per_step_per_rank={"a_group_step_host_arrays": int(N * FN * 4 + E * FE * 4 + N * O * 4) + params_b,
                                             "b_group_step_datapoint": params_b, "of_these_set_params": params_b},
                resident_trajectory_bytes_per_rank=[int(T * n * O * 4) for n in own])


out = {"workload": f"L=128 mps=15 fp32, T={T} frames, {ITERS} iterations per block, set_params with new parameters before every step, "
                   f"{ROUNDS} rounds, ranks share device 0", "device": torch.cuda.get_device_name(0), "runs": []}
for name, pos, (s, r) in meshes():
    for P in (2, 4):
        out["runs"].append(run(name, pos, s, r, P))
        print(json.dumps(out["runs"][-1]), flush=True)
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
