"""A 100-save rollout on the cylinder mesh (2 000 points, L = 128, mps = 15; bench.py's rollout_100_saves workload) through Engine.rollout
with the method given as a tableau (mgn_rollout_erk) beside the two solvers mgn_rollout names itself, in one process on one engine:
the Euler and Tsit5 tableaux against MGN_SOLVER_EULER / MGN_SOLVER_TSIT5_FIXED / MGN_SOLVER_TSIT5 (the same loops: the same time), then
Heun, RK4, BS3 and DP5 with fixed steps of saves_dt and, where there is an embedded pair, adaptive.  Every loop replays the same
captured right-hand side, so the time per right-hand side should agree across the fixed-step rows.  Wall times of whole calls, host
arrays in and out included; after one warm-up call each, the median of the repeats.

    python3 tools/rollout_erk_timing.py [repeats=5]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch  # noqa: F401  (before the engine's first HIP call)
import mgn_amd
import bench

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
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


def timed(solver, **kw):
    call = lambda: eng.rollout(solver, vel, onehot, ef, 0.0, 1.0, 0.01, 101, val_mask=vm, **kw)      # noqa: E731
    call()                                # warm-up: arenas, weight layouts, graph capture
    ts = []
    for _ in range(REPS):
        t = time.perf_counter()
        _, st = call()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)), st, (min(ts), max(ts))


T = mgn_amd.erk_tableau
FIXED, ADAPTIVE = dict(dt=0.01, adaptive=False), dict()
print(f"cylinder N={N} E={s.size} L={L} mps={MPS}, t in [0, 1], 101 saves of 0.01; {REPS} repeats, median (min .. max)")
for label, solver, kw in (("Euler (solver 0)", "Euler", FIXED), ("Euler tableau", T("Euler"), FIXED),
                          ("Tsit5 fixed (solver 2)", "Tsit5", FIXED), ("Tsit5 tableau, fixed", T("Tsit5"), FIXED),
                          ("Tsit5 adaptive (solver 1)", "Tsit5", ADAPTIVE), ("Tsit5 tableau, adaptive", T("Tsit5"), ADAPTIVE),
                          ("Heun, fixed", "Heun", FIXED), ("RK4, fixed", "RK4", FIXED), ("BS3, fixed", "BS3", FIXED), ("DP5, fixed", "DP5", FIXED),
                          ("BS3, adaptive", "BS3", ADAPTIVE), ("DP5, adaptive", "DP5", ADAPTIVE)):
    med, st, (lo, hi) = timed(solver, **kw)
    print(f"{label}: {med * 1e3:.2f} ms ({lo * 1e3:.2f} .. {hi * 1e3:.2f}), {st['n_accept']} steps, {st['n_reject']} rejected, "
          f"{st['n_rhs']} right-hand sides, {med / st['n_rhs'] * 1e6:.1f} us per right-hand side")
eng.close()
