"""Derivative-training loop on the cylinder-sized mesh of bench.py --full: 100 iterations, new parameters before every step.
(a) the host way: reference_api.init_train_step_derivative (NumPy) + Engine.step on host arrays
(b) Engine.step on precomputed device tensors (the floor)
(c) Engine.step_datapoint, without / with accumulate, gradients to a host array (as a) and to a device tensor (as b)
Alternating blocks, three rounds; ms per iteration, host clock around calls that end in a stream synchronise."""
import json, os, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "oracle"))
import mgn_amd
import mgn_oracle as orc
from mgn_amd import reference_api as ra

L, MPS, FN, FE, O = 128, 15, 9, 3, 2
ITERS, ROUNDS, T = 100, 3, 101
pos, cells, ntype, vel = mgn_amd.synth.mesh_cyl(1234, 2000)
s, r = mgn_amd.synth.cells_to_edges(cells)
N, E = pos.shape[0], s.size
rng = np.random.default_rng(0)
frames = (vel[None] + 0.01 * np.cumsum(rng.standard_normal((T, N, O)), 0)).astype(np.float32)
onehot = ra.one_hot(ntype, FN - O, -int(ntype.min())) if ntype.max() - ntype.min() < FN - O else ra.one_hot(ntype % (FN - O), FN - O)
rel = pos[s] - pos[r]
ef_raw = np.concatenate([rel, np.linalg.norm(rel, axis=1, keepdims=True)], 1).astype(np.float32)
mask = np.nonzero(np.isin(ntype, [0, 5]))[0].astype(np.int32)
if mask.size == 0:
    mask = np.arange(N, dtype=np.int32)
ps = orc.init_params(FN, FE, O, L, 2, MPS, seed=1234, ln_jitter=0.1)
dt = np.float32(0.01)


class Mgn:
    pass


def mirror_mgn(online):
    m = Mgn()
    if online:
        m.n_norm = {"velocity": ra.NormaliserOnline(O), "node_type": ra.NormaliserOfflineMinMax(0.0, 1.0)}
        m.e_norm = ra.NormaliserOnline(FE)
        m.o_norm = {"velocity": ra.NormaliserOnline(O)}
    else:
        m.n_norm = {"velocity": ra.NormaliserOfflineMeanStd(frames.mean((0, 1)), frames.std((0, 1))), "node_type": ra.NormaliserOfflineMinMax(0.0, 1.0)}
        m.e_norm = ra.NormaliserOfflineMeanStd(ef_raw.mean(0), ef_raw.std(0))
        d = (frames[1:] - frames[:-1]) / dt
        m.o_norm = {"velocity": ra.NormaliserOfflineMeanStd(d.mean((0, 1)), d.std((0, 1)))}
    return m


frozen = mirror_mgn(False)
vs, vsh = frozen.n_norm["velocity"].affine(O)
norms = dict(node=(np.concatenate([vs, np.ones(FN - O, np.float32)]), np.concatenate([vsh, np.zeros(FN - O, np.float32)])),
             edge=frozen.e_norm.affine(FE), out=frozen.o_norm["velocity"].inverse_affine(O))
data = {"velocity": frames[:-1], "target|velocity": frames[1:]}

eng = mgn_amd.Engine(FN, FE, O, L, 2, MPS, device=0)
eng.set_params(ps)
eng.set_norms(**norms)
eng.set_graph(s, r, N)
eng.set_trajectory(frames, dt=dt, node_type_onehot=onehot, ef_raw=ef_raw)
gs_host = np.zeros(eng.param_count, np.float32)
gs_dev = torch.zeros(eng.param_count, device="cuda:0")
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
pre = [tuple(dev(a) for a in eng.datapoint_export(t)) for t in range(ITERS)]
state = {"ps": ps.copy()}


def new_params():
    state["ps"] *= np.float32(1.00001)
    eng.set_params(state["ps"])


def block_a(mgn):
    def run():
        for t in range(ITERS):
            new_params()
            g, tq = ra.init_train_step_derivative(mgn, data, {"dt": float(dt)}, ["velocity"], ["velocity"], onehot, ef_raw, s, r, t)
            eng.step(g.nf, g.ef, tq, mask, out=gs_host)
    return run


def block_b():
    for t in range(ITERS):
        new_params()
        eng.step(*pre[t], mask, out=gs_dev)


def block_c(acc, out):
    def run():
        for t in range(ITERS):
            new_params()
            eng.step_datapoint(t, mask, accumulate=acc, out=out)
    return run


def online_reset():
    eng.set_norms(**norms)
    eng.online_norms()


blocks = [("a_host_build_graph_frozen", block_a(frozen), None),
          ("a_host_build_graph_online", None, "mirror"),
          ("b_step_device_tensors", block_b, None),
          ("c_step_datapoint_host_grads", block_c(False, gs_host), None),
          ("c_step_datapoint_device_grads", block_c(False, gs_dev), None),
          ("c_step_datapoint_accumulate_host_grads", block_c(True, gs_host), "online"),
          ("c_step_datapoint_accumulate_device_grads", block_c(True, gs_dev), "online")]
res = {k: [] for k, _, _ in blocks}
for rnd in range(ROUNDS + 1):                      # round 0 warms every path (eager, capture, replay)
    for name, fn, mode in blocks:
        if mode == "mirror":
            fn = block_a(mirror_mgn(True))
        if mode == "online":
            online_reset()
        else:
            eng.online_norms(node=False, edge=False, out=False)
            eng.set_norms(**norms)
        eng.synchronize()
        t0 = time.perf_counter()
        fn()
        eng.synchronize()
        ms = (time.perf_counter() - t0) / ITERS * 1e3
        if rnd:
            res[name].append(ms)
out = {"workload": f"M-cyl N={N} E={E} L=128 mps=15 fp32, {ITERS} iterations per block, set_params with new parameters before every step, {ROUNDS} rounds",
       "device": torch.cuda.get_device_name(0), "ms_per_iteration": {k: {"median": float(np.median(v)), "all": [round(x, 4) for x in v]} for k, v in res.items()}}
m = {k: v["median"] for k, v in out["ms_per_iteration"].items()}
out["ratios"] = {"c_over_a": m["c_step_datapoint_host_grads"] / m["a_host_build_graph_frozen"],
                 "c_over_b": m["c_step_datapoint_device_grads"] / m["b_step_device_tensors"],
                 "c_acc_over_a_online": m["c_step_datapoint_accumulate_host_grads"] / m["a_host_build_graph_online"],
                 "c_acc_over_b": m["c_step_datapoint_accumulate_device_grads"] / m["b_step_device_tensors"]}
print(json.dumps(out))
