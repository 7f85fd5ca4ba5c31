"""Per-datapoint time of the derivative-training loop on the cylinder-sized mesh of bench.py (M-cyl, about 2 000 nodes, L = 128,
15 steps): a loop of Engine.step_datapoint against Engine.step_datapoints at B = 2, 4, 8, 16, 32.  Gradients go to a device tensor
and set_params with new parameters precedes every call, as in a real loop.  One engine per batch size (a handle keeps two companion
sizes), every shape warmed (eager, capture, replay), the variants alternated in one process, at least a second per variant and round,
each block ending in a synchronise; the spread over the rounds is reported.  Also: the device memory each batch size's companion
took (graph, weights and training arena; hipMemGetInfo before and after its first call)."""
import json, os, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "oracle"))
import mgn_amd
import mgn_oracle as orc
from mgn_amd import reference_api as ra

L, MPS, FN, FE, O = 128, 15, 9, 3, 2
ROUNDS, T, MIN_S = 3, 101, 1.0
BATCHES = (2, 4, 8, 16, 32)
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
d = (frames[1:] - frames[:-1]) / dt
vn = ra.NormaliserOfflineMeanStd(frames.mean((0, 1)), frames.std((0, 1)))
vs, vsh = vn.affine(O)
norms = dict(node=(np.concatenate([vs, np.ones(FN - O, np.float32)]), np.concatenate([vsh, np.zeros(FN - O, np.float32)])),
             edge=ra.NormaliserOfflineMeanStd(ef_raw.mean(0), ef_raw.std(0)).affine(FE),
             out=ra.NormaliserOfflineMeanStd(d.mean((0, 1)), d.std((0, 1))).inverse_affine(O))
gs_dev = torch.zeros(orc.param_count(FN, FE, O, L, 2, MPS), device="cuda:0")
state = {"ps": ps.copy()}


def engine():
    eng = mgn_amd.Engine(FN, FE, O, L, 2, MPS, device=0)
    eng.set_params(ps)
    eng.set_norms(**norms)
    eng.set_graph(s, r, N)
    eng.set_trajectory(frames, dt=dt, node_type_onehot=onehot, ef_raw=ef_raw)
    return eng


def variant(eng, B):
    """one call: new parameters, then B datapoints (B = 0: the single entry point); returns the datapoints it consumed"""
    pos_ = {"t": 0}

    def call():
        state["ps"] *= np.float32(1.00001)
        eng.set_params(state["ps"])
        t0 = pos_["t"]
        nb = max(B, 1)
        ts = [(t0 + i) % (T - 1) for i in range(nb)]
        pos_["t"] = (t0 + nb) % (T - 1)
        if B == 0:
            eng.step_datapoint(ts[0], mask, out=gs_dev)
        else:
            eng.step_datapoints(ts, mask, out=gs_dev)
        return nb
    return call


engines = {0: engine()}
variants = {"loop_step_datapoint": (engines[0], variant(engines[0], 0))}
companion_bytes = {}
for B in BATCHES:
    engines[B] = engine()
    call = variant(engines[B], B)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    call()
    engines[B].synchronize()
    companion_bytes[B] = int(free0 - torch.cuda.mem_get_info(0)[0])
    variants[f"step_datapoints_B{B}"] = (engines[B], call)
for eng, call in variants.values():                  # every shape: eager, capture, replay
    for _ in range(4):
        call()
    eng.synchronize()
calls = {}
for name, (eng, call) in variants.items():           # how many calls fill MIN_S seconds
    eng.synchronize()
    t0 = time.perf_counter()
    n = 0
    while time.perf_counter() - t0 < 0.25:
        call(); n += 1
    eng.synchronize()
    calls[name] = max(4, int(n * MIN_S / 0.25 * 1.1) + 1)
res = {k: [] for k in variants}
for rnd in range(ROUNDS):
    for name, (eng, call) in variants.items():
        eng.synchronize()
        t0 = time.perf_counter()
        dps = 0
        for _ in range(calls[name]):
            dps += call()
        eng.synchronize()
        el = time.perf_counter() - t0
        res[name].append({"ms_per_datapoint": el / dps * 1e3, "ms_per_call": el / calls[name] * 1e3, "seconds": el})
base = float(np.median([x["ms_per_datapoint"] for x in res["loop_step_datapoint"]]))
table = {}
for name, v in res.items():
    per = [x["ms_per_datapoint"] for x in v]
    table[name] = {"ms_per_datapoint_median": float(np.median(per)), "min": float(min(per)), "max": float(max(per)),
                   "ms_per_call_median": float(np.median([x["ms_per_call"] for x in v])), "calls_per_round": calls[name],
                   "seconds_per_round": [round(x["seconds"], 3) for x in v], "loop_over_this": base / float(np.median(per))}
out = {"workload": f"M-cyl N={N} E={E} L=128 mps=15 fp32, gradients to a device tensor, set_params with new parameters before every call, {ROUNDS} rounds of >= {MIN_S} s per variant",
       "device": torch.cuda.get_device_name(0), "per_datapoint": table,
       "companion_device_bytes": {f"B{B}": v for B, v in companion_bytes.items()}}
print(json.dumps(out))
