"""A 100-save rollout on the cylinder mesh (2 000 points, L = 128, mps = 15; bench.py's rollout_100_saves workload) through Engine.rollout:
fixed-step Tsit5 at dt = saves_dt (MGN_SOLVER_TSIT5_FIXED: 100 steps, 601 right-hand sides) beside fixed-step Euler (100 steps, one
right-hand side each) and adaptive Tsit5, in one process on one engine.  Both fixed-step loops replay the same captured right-hand
side, so their time per right-hand side should agree.  Wall times of whole calls, host arrays in and out included; after one warm-up
call each, the median of the repeats.

    python3 tools/rollout_tsit5_fixed_timing.py [repeats=7]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch  # noqa: F401  (before the engine's first HIP call)
import mgn_amd
import bench

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
FN, FE, O, L, MPS = 9, 3, 2, 128, 15

pos, cells, ntype, vel = mgn_amd.synth.mesh_cyl(1234, 2000)
s, r = mgn_amd.synth.cells_to_edges(cells)
N = pos.shape[0]
eng = mgn_amd.Engine(FN, FE, O, L, 2, MPS)
eng.set_params(bench.glorot_params())
eng.set_graph(s, r, N)
onehot = np.eye(7, dtype=np.float32)[ntype]
rel = pos[s] - pos[r]
ef = np.concatenate([rel, np.linalg.norm(rel, axis=1, keepdims=True)], 1).astype(np.float32)
eng.set_norms(node=(np.ones(FN, np.float32), np.zeros(FN, np.float32)),
              edge=(1.0 / np.maximum(ef.std(0), 1e-8), -ef.mean(0) / np.maximum(ef.std(0), 1e-8)),
              out=(np.full(O, 0.05, np.float32), np.zeros(O, np.float32)))
vm = np.isin(ntype, [0, 5]).astype(np.float32)


def timed(name, **kw):
    call = lambda: eng.rollout(name, vel, onehot, ef, 0.0, 1.0, 0.01, 101, val_mask=vm, **kw)
    call()                                # warm-up: arenas, weight layouts, graph capture
    ts = []
    for _ in range(REPS):
        t = time.perf_counter()
        _, st = call()
        ts.append(time.perf_counter() - t)
    med = float(np.median(ts))
    return med, st, (min(ts), max(ts))


print(f"cylinder N={N} E={s.size} L={L} mps={MPS}, t in [0, 1], 101 saves of 0.01; {REPS} repeats, median (min .. max)")
for label, name, kw in (("Euler, dt = 0.01", "Euler", dict(dt=0.01)),
                        ("Tsit5, fixed steps of 0.01", "Tsit5", dict(dt=0.01, adaptive=False)),
                        ("Tsit5, adaptive", "Tsit5", dict())):
    med, st, (lo, hi) = timed(name, **kw)
    print(f"{label}: {med * 1e3:.2f} ms ({lo * 1e3:.2f} .. {hi * 1e3:.2f}), {st['n_accept']} steps, {st['n_reject']} rejected, "
          f"{st['n_rhs']} right-hand sides, {med / st['n_rhs'] * 1e6:.1f} us per right-hand side")
eng.close()
