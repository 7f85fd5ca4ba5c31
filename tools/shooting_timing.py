"""One training step of MultipleShooting (reference src/strategies.jl:312-383) on the cylinder mesh (mesh_cyl, ~2 000 nodes, L = 128,
mps = 15): train_step_multiple_shooting's per-window loop (one mgn_solver_grad / mgn_solver_grad_tsit5 call per window) against the
batched call (mgn_shooting_grad: windows with the same step plan solved as one block-diagonal batch), for Euler and fixed-step Tsit5.
Device-synchronised wall time per MultipleShooting step (median of the repeats after one warm-up call), windows per pass, and the
agreement of loss and gradient.

    python3 tools/shooting_timing.py [T=101] [interval_size=10] [repeats=3]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch  # noqa: F401  (before the engine's first HIP call)
import mgn_amd
from mgn_amd import reference_api as ra
import bench

ARGS = sys.argv[1:]
T = int(ARGS[0]) if ARGS else 101
INTERVAL = int(ARGS[1]) if len(ARGS) > 1 else 10
REPS = int(ARGS[2]) if len(ARGS) > 2 else 3
DT = 0.01


def timed(fn):
    out = fn()                          # warm-up: arenas, companion graph, weight packing, graph capture
    ts = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)), out


def main():
    pos, cells, ntype, vel = mgn_amd.synth.mesh_cyl(1234, 2000)
    s, r = mgn_amd.synth.cells_to_edges(cells)
    N = pos.shape[0]
    eng = mgn_amd.Engine(9, 3, 2, 128, 2, 15)
    eng.set_params(bench.glorot_params())
    eng.set_graph(s, r, N)
    eng.set_norms(node=(np.r_[np.full(2, 2.5), np.ones(7)].astype(np.float32), np.zeros(9, np.float32)),
                  out=(np.full(2, 0.05, np.float32), np.zeros(2, np.float32)))
    onehot = np.eye(7, dtype=np.float32)[np.clip(ntype, 0, 6)]
    ef = np.concatenate([pos[s] - pos[r], np.linalg.norm(pos[s] - pos[r], axis=1, keepdims=True)], axis=1).astype(np.float32)
    rng = np.random.default_rng(0)
    gt = (vel[None] * (1.0 + 0.05 * rng.standard_normal((T, N, 2)))).astype(np.float32)
    vm = np.isin(ntype, [0, 5]).astype(np.float32)
    windows = ra.multiple_shooting_ranges(T, INTERVAL)
    res = {"mesh_nodes": N, "mesh_edges": int(s.size), "T": T, "interval_size": INTERVAL, "windows": len(windows)}
    for solver in ("Euler", "Tsit5"):
        args = (eng, gt, onehot, ef, 0.0, DT, (T - 1) * DT, INTERVAL, 0.5)
        kw = dict(val_mask=vm, solver=solver, adaptive=False)
        t_loop, (gs_l, loss_l) = timed(lambda: ra.train_step_multiple_shooting(*args, **kw))
        t_bat, (gs_b, loss_b) = timed(lambda: ra.train_step_multiple_shooting(*args, batched=True, **kw))
        st = eng.last_shooting
        rel = float(np.linalg.norm(gs_b - gs_l) / np.linalg.norm(gs_l))
        res[solver] = {"loop_ms": round(t_loop * 1e3, 2), "batched_ms": round(t_bat * 1e3, 2), "speedup": round(t_loop / t_bat, 2),
                       "n_groups": st["n_groups"], "n_passes": st["n_passes"], "windows_per_pass": round(len(windows) / st["n_passes"], 2),
                       "loss_rel_diff": abs(loss_b - loss_l) / abs(loss_l), "grad_rel_l2": rel}
        print(f"{solver:6s} loop {t_loop * 1e3:9.2f} ms   batched {t_bat * 1e3:9.2f} ms   x{t_loop / t_bat:5.2f}   "
              f"{st['n_passes']} passes / {len(windows)} windows   loss {res[solver]['loss_rel_diff']:.2e}   grad {rel:.2e}", flush=True)
    eng.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
