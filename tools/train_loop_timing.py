"""The reference's training loop (src/MeshGraphNets.jl:364-378: step!, Optimisers.update, new parameters) on the cylinder-sized mesh of
bench.py, L = 128, mps = 15, resident trajectory, three ways:
(a) step_datapoint to a host array, checkpoint.Adam.update on the host, set_params          (entry points every version has)
(b) step_datapoint(out = device), torch.optim.Adam on a device tensor, set_params_dev
(c) step_datapoint(out = device), adam_update
The arms alternate in one process, ROUNDS rounds of ITERS iterations after a warm-up round; a window ends in synchronize(); ms per
iteration.  On a tree without the device-side calls only (a) runs -- the figure to hold the others against:
    python tools/train_loop_timing.py [--iters 60] [--rounds 5] [--trace-arm c]
--trace-arm X: only arm X, once (for a kernel trace of one arm alone)."""
import argparse, json, os, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "oracle"))
import mgn_amd
import mgn_oracle as orc
from mgn_amd import reference_api as ra
from mgn_amd.checkpoint import Adam

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=60)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--trace-arm", default=None)
args = ap.parse_args()

L, MPS, FN, FE, O = 128, 15, 9, 3, 2
T = 101
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
HAVE_DEV = hasattr(mgn_amd.Engine, "adam_update")


def engine():
    e = mgn_amd.Engine(FN, FE, O, L, 2, MPS, device=0)
    e.set_params(ps0)
    e.set_norms(**norms)
    e.set_graph(s, r, N)
    e.set_trajectory(frames, dt=dt, node_type_onehot=onehot, ef_raw=ef_raw)
    return e


class ArmA:
    def __init__(self):
        self.e, self.opt = engine(), Adam()
        self.ps, self.gs = ps0.copy(), np.zeros(ps0.size, np.float32)
        self.st = self.opt.setup(self.ps)

    def it(self, t):
        self.e.step_datapoint(t, mask, out=self.gs)
        self.st, self.ps = self.opt.update(self.st, self.ps, self.gs)
        self.e.set_params(self.ps)


class ArmB:
    def __init__(self):
        self.e = engine()
        self.stream = torch.cuda.Stream()                 # torch's optimiser and the engine on one stream (not the legacy one: the engine replays launch graphs)
        self.e.set_stream(self.stream.cuda_stream)
        self.p = torch.from_numpy(ps0.copy()).to("cuda:0")
        self.p.grad = torch.zeros_like(self.p)
        self.opt = torch.optim.Adam([self.p], lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
        torch.cuda.synchronize()
        self.e.set_params_dev(self.p)

    def it(self, t):
        with torch.cuda.stream(self.stream):
            self.e.step_datapoint(t, mask, out=self.p.grad)
            self.opt.step()
            self.e.set_params_dev(self.p)


class ArmC:
    def __init__(self):
        self.e = engine()
        self.gs = torch.zeros(ps0.size, device="cuda:0")
        self.e.set_params_dev(torch.from_numpy(ps0).to("cuda:0"))
        self.e.adam_init(1e-3, (0.9, 0.999), 1e-8)

    def it(self, t):
        self.e.step_datapoint(t, mask, out=self.gs)
        self.e.adam_update(self.gs)


kinds = {"a": ArmA}
if HAVE_DEV:
    kinds.update(b=ArmB, c=ArmC)
if args.trace_arm:
    kinds = {args.trace_arm: kinds[args.trace_arm]}
arms = {k: v() for k, v in kinds.items()}
rounds = 1 if args.trace_arm else args.rounds
res = {k: [] for k in arms}
for rnd in range(rounds + 1):                     # round 0 warms every arm's shapes (eager, capture, replay)
    for k, arm in arms.items():
        arm.e.synchronize(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(args.iters):
            arm.it(i % (T - 1))
        arm.e.synchronize(); torch.cuda.synchronize()
        if rnd:
            res[k].append((time.perf_counter() - t0) / args.iters * 1e3)
out = {"workload": f"M-cyl N={N} E={E} L=128 mps=15 fp32, resident trajectory, {args.iters} iterations per window, {rounds} rounds, arms alternating",
       "device": torch.cuda.get_device_name(0), "device_side_calls": HAVE_DEV,
       "ms_per_iteration": {k: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "all": [round(x, 4) for x in v]}
                            for k, v in res.items()}}
print(json.dumps(out))
