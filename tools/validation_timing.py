"""One validation trajectory (_validation_step, reference src/strategies.jl:111-134): mgn_rollout_eval without the solution
(Engine.rollout_eval: errors reduced on the device, nothing of the size of the solution held or downloaded, the ground truth uploaded
once as the inflow data) against the route it replaces on the same engine -- Engine.rollout, then the NumPy reduction
`mean((prediction - gt) .^ 2; dims = 3)` and `mean(error[mask])`.  The cylinder mesh (mesh_cyl, ~2 000 nodes) and a grid mesh, L = 128,
mps = 15, Euler (dt = the save spacing) and adaptive Tsit5.  The two routes alternate inside one process after a warm-up call each;
wall time of a whole call (it ends in a device synchronisation), medians and the spread.  Also the device bytes that depend on the
route: mgn_rollout's [n_saves][N][O] save buffer against mgn_rollout_eval's accumulator, partials and outputs.

    python3 tools/validation_timing.py [--saves 101] [--reps 5] [--grid NX NY] [--grid-reps 2] [--grid-solvers Euler]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch  # noqa: F401  (before the engine's first HIP call)
import mgn_amd
import bench

DT = 0.01


def host_validation(eng, solver, x0, onehot, ef, gt, kw, mask):
    pred, _ = eng.rollout(solver, x0, onehot, ef, **kw)
    error = np.mean((pred - gt[:pred.shape[0]]) ** 2, axis=0)         # Float32, as the reference's arrays are
    return float(np.mean(error.reshape(-1)[mask]))


def route_bytes(N, O, n_saves, n_sel):
    """Bytes of the call's device arena that differ between the routes (state, stages, frames, mask, encoded edges are common)."""
    n = N * O
    blocks = min(max((N + 255) // 256, 1), 1024)
    vblocks = min(max((max(n_sel, 1) + 255) // 256, 1), 1024)
    return {"rollout_save_buffer": n_saves * n * 4,
            "rollout_eval": n * 8 + n_saves * blocks * O * 8 + n_sel * 8 + vblocks * 8 + n_saves * O * 8 + n * 4}


def measure(name, pos, cells, ntype, vel, n_saves, reps, solvers):
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
    gt = (vel[None] * (1.0 + 0.05 * rng.standard_normal((n_saves, N, 2)).astype(np.float32))).astype(np.float32)
    vm = np.isin(ntype, [0, 5]).astype(np.float32)
    im = (ntype == 4).astype(np.uint8)
    mask = np.nonzero(np.isin(ntype, [0, 5]))[0].astype(np.int32)
    res = {"mesh": name, "nodes": N, "edges": int(s.size), "n_saves": n_saves, "bytes": route_bytes(N, 2, n_saves, int(mask.size))}
    for solver in solvers:
        kw = dict(t0=0.0, t1=(n_saves - 1) * DT, saves_dt=DT, n_saves=n_saves, dt=DT if solver == "Euler" else 0.0, val_mask=vm,
                  inflow_mask=im if im.any() else None, inflow_data=gt if im.any() else None, inflow_rule="tolerant")
        routes = {"host": lambda: host_validation(eng, solver, gt[0], onehot, ef, gt, kw, mask),
                  "native": lambda: eng.rollout_eval(solver, gt[0], onehot, ef, gt, sel=mask, **kw)["val_loss"]}
        val = {k: f() for k, f in routes.items()}                       # warm-up: arenas, weight packing, graph capture
        ts = {k: [] for k in routes}
        for _ in range(reps):
            for k, f in routes.items():                                  # alternating: both see the same machine
                torch.cuda.synchronize()
                t = time.perf_counter()
                f()
                torch.cuda.synchronize()
                ts[k].append(time.perf_counter() - t)
        med = {k: float(np.median(v)) for k, v in ts.items()}
        res[solver] = {"host_ms": round(med["host"] * 1e3, 2), "native_ms": round(med["native"] * 1e3, 2),
                       "speedup": round(med["host"] / med["native"], 3),
                       "host_ms_min_max": [round(min(ts["host"]) * 1e3, 2), round(max(ts["host"]) * 1e3, 2)],
                       "native_ms_min_max": [round(min(ts["native"]) * 1e3, 2), round(max(ts["native"]) * 1e3, 2)],
                       "val_loss_rel_diff": abs(val["native"] - val["host"]) / abs(val["host"])}
        print(f"{name:8s} N={N:8d} {solver:6s} rollout + NumPy {med['host'] * 1e3:10.2f} ms   rollout_eval {med['native'] * 1e3:10.2f} ms   "
              f"x{med['host'] / med['native']:5.3f}   val_loss diff {res[solver]['val_loss_rel_diff']:.2e}", flush=True)
    eng.close()
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--saves", type=int, default=101)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--grid", type=int, nargs=2, default=[1000, 1000])
    ap.add_argument("--grid-reps", type=int, default=2)
    ap.add_argument("--grid-solvers", nargs="*", default=["Euler"])
    a = ap.parse_args()
    pos, cells, ntype, vel = mgn_amd.synth.mesh_cyl(1234, 2000)
    measure("cylinder", pos, cells, ntype, vel, a.saves, a.reps, ("Euler", "Tsit5"))
    if a.grid[0] > 0 and a.grid_solvers:
        pos, cells = mgn_amd.synth.grid_mesh(a.grid[0], a.grid[1], 1234)
        rng = np.random.default_rng(1)
        ntype = rng.choice([0, 4, 5, 6], pos.shape[0], p=[0.85, 0.05, 0.05, 0.05]).astype(np.int32)
        vel = rng.standard_normal((pos.shape[0], 2)).astype(np.float32)
        measure("grid", pos, cells, ntype, vel, a.saves, a.grid_reps, a.grid_solvers)


if __name__ == "__main__":
    main()
