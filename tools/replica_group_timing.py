"""One training iteration on a minibatch of B = 8 resident datapoints (step_datapoints + adam_update, nothing downloaded) on the
cylinder-sized mesh of bench.py, L = 128, mps = 15, three ways:
(e)  a plain Engine: step_datapoints(out = device tensor), adam_update(that tensor)
(g1) a replica group of one: GroupEngine.step_datapoints(want_grads=False), adam_update()
(g2) a replica group of two, both replicas on device 0 (they share the device: expected to be no faster)
and (h) the thread hand-off of a group call alone: GroupEngine.synchronize() on the idle group of one, per call.
The arms alternate in one process, ROUNDS rounds of ITERS iterations after a warm-up round; a window ends in synchronize(); ms per
iteration.
    python tools/replica_group_timing.py [--iters 40] [--rounds 5] [--batch 8]"""
import argparse, json, os, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "oracle"))
import mgn_amd
import mgn_oracle as orc
from mgn_amd import reference_api as ra

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=40)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--batch", type=int, default=8)
args = ap.parse_args()

L, MPS, FN, FE, O = 128, 15, 9, 3, 2
T = 101
B = args.batch
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
ps0 = orc.init_params(FN, FE, O, L, 2, MPS, seed=1234, ln_jitter=0.1).astype(np.float32)
dt = np.float32(0.01)
d = (frames[1:] - frames[:-1]) / dt
norms = dict(node=(np.concatenate([1 / frames.std((0, 1)), np.ones(FN - O)]).astype(np.float32),
                   np.concatenate([-frames.mean((0, 1)) / frames.std((0, 1)), np.zeros(FN - O)]).astype(np.float32)),
             edge=((1 / ef_raw.std(0)).astype(np.float32), (-ef_raw.mean(0) / ef_raw.std(0)).astype(np.float32)),
             out=(d.std((0, 1)).astype(np.float32), d.mean((0, 1)).astype(np.float32)))


def setup(e):
    e.set_norms(**norms)
    e.set_graph(s, r, N)
    e.set_trajectory(frames, dt=dt, node_type_onehot=onehot, ef_raw=ef_raw)
    e.set_params_dev(ps0)
    e.adam_init(1e-3, (0.9, 0.999), 1e-8)
    return e


def batch(i):
    return [(i * B + b) % (T - 1) for b in range(B)]


class Plain:
    def __init__(self):
        self.e = setup(mgn_amd.Engine(FN, FE, O, L, 2, MPS, device=0))
        self.gs = torch.zeros(ps0.size, device="cuda:0")

    def it(self, i):
        self.e.step_datapoints(batch(i), mask, out=self.gs)
        self.e.adam_update(self.gs)


class Group:
    def __init__(self, P):
        self.e = setup(mgn_amd.GroupEngine(FN, FE, O, L, 2, MPS, devices=[0] * P, replicas=True))

    def it(self, i):
        self.e.step_datapoints(batch(i), mask, want_grads=False)
        self.e.adam_update()


arms = {"engine": Plain(), "replicas_1": Group(1), "replicas_2": Group(2)}
res = {k: [] for k in arms}
for rnd in range(args.rounds + 1):                # round 0 warms every arm's shapes (eager, capture, replay)
    for k, arm in arms.items():
        arm.e.synchronize(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(args.iters):
            arm.it(i)
        arm.e.synchronize(); torch.cuda.synchronize()
        if rnd:
            res[k].append((time.perf_counter() - t0) / args.iters * 1e3)
g1 = arms["replicas_1"].e
hand = []
for rnd in range(args.rounds + 1):
    t0 = time.perf_counter()
    for _ in range(2000):
        g1.synchronize()
    if rnd:
        hand.append((time.perf_counter() - t0) / 2000 * 1e3)
p = [arms["replicas_2"].e.get_params_dev(k) for k in range(2)]
out = {"workload": f"M-cyl N={N} E={E} L=128 mps=15 fp32, resident trajectory, B={B}, {args.iters} iterations per window, {args.rounds} rounds, arms alternating",
       "device": torch.cuda.get_device_name(0), "replicas_agree": bool(np.array_equal(p[0].view(np.uint32), p[1].view(np.uint32))),
       "ms_per_iteration": {k: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "all": [round(x, 4) for x in v]}
                            for k, v in res.items()},
       "ms_per_group_call_hand_off": {"median": float(np.median(hand)), "min": float(min(hand)), "max": float(max(hand))}}
print(json.dumps(out))
