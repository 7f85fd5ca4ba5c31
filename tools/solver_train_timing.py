"""One training step of SolverTraining with Euler() (reference src/strategies.jl:175-196, 257-292): the native call (mgn_solver_grad)
against the host composition reference_api.solver_training_euler(ode_step, ode_vjp) -- one mgn_ode_step per step forward, one
mgn_ode_vjp (upload of the statics, synchronise, gradient copy-out) plus a float64 NumPy add per step backward -- in one process, on the
cylinder mesh (L = 128, mps = 15, K Euler steps); then the native call alone on a ~125 k-node grid at a small K.  Device-synchronised
wall times (median of the repeats after one warm-up call).

With --tsit5: one SolverTraining step with Tsit5() instead -- the native mgn_solver_grad_tsit5 (adaptive, tstops = saves) against the
host composition reference_api.solver_training_tsit5(ode_step, ode_vjp) fed the step sequence the native call recorded, on the
cylinder mesh over K save intervals of 0.01; ms per accepted step and the bytes of the stored stage inputs.

    python3 tools/solver_train_timing.py [K_cyl=100] [K_125k=10] [repeats=3]
    python3 tools/solver_train_timing.py --tsit5 [K_cyl=20] [repeats=3]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch  # noqa: F401  (before the engine's first HIP call)
import mgn_amd
from mgn_amd import reference_api as ra
import bench

TSIT5 = "--tsit5" in sys.argv[1:]
ARGS = [a for a in sys.argv[1:] if a != "--tsit5"]
K_CYL = int(ARGS[0]) if ARGS else (20 if TSIT5 else 100)
K_BIG = 0 if TSIT5 else (int(ARGS[1]) if len(ARGS) > 1 else 10)
REPS = int(ARGS[1 if TSIT5 else 2]) if len(ARGS) > (1 if TSIT5 else 2) else 3
DT = 0.01


def setup(pos, cells, ntype, vel, K):
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
    gt = (vel[None] * (1.0 + 0.05 * rng.standard_normal((K + 1, N, 2)))).astype(np.float32)
    vm = np.isin(ntype, [0, 5]).astype(np.float32)
    return eng, onehot, ef, gt, vm, N, s.size


def timed(fn):
    ts = []
    out = fn()                          # warm-up: arenas, weight packing, graph capture
    for _ in range(REPS):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)), out


def native(eng, onehot, ef, gt, vm, K):
    ns = np.full(2, 2.5, np.float32)
    return lambda: eng.solver_grad(gt[0], onehot, ef, gt, 0.0, K * DT, DT, DT, K + 1, val_mask=vm, loss_scale=ns)


def tsit5_mode():
    pos, cells, ntype, vel = mgn_amd.synth.mesh_cyl(1234, 2000)
    eng, onehot, ef, gt, vm, N, E = setup(pos, cells, ntype, vel, K_CYL)
    ns = np.full(2, 2.5, np.float32)
    t1 = float(np.float32(K_CYL * DT))
    t_nat, (gs, loss, st) = timed(lambda: eng.solver_grad_tsit5(gt[0], onehot, ef, gt, 0.0, t1, DT, K_CYL + 1, val_mask=vm, loss_scale=ns))
    K = st["n_accept"]
    # the save each state is: the solve stops on every save point
    times = list(st["step_t"]) + [t1]
    save_step = [next((n for n, t in enumerate(times) if abs(float(np.float32(s * np.float32(DT))) - t) <= 1e-9 * abs(t) + 1e-12), K)
                 for s in range(K_CYL + 1)]
    host = lambda: ra.solver_training_tsit5(lambda x: eng.ode_step(x, onehot, ef, vm),
                                            lambda x, lam: eng.ode_vjp(x, onehot, ef, lam, val_mask=vm)[:2], gt[0], gt, st["step_t"],
                                            st["step_h"], val_mask=vm, n_scale=ns, save_step=save_step)
    t_host, (gs_h, loss_h, _) = timed(host)
    rel = float(np.linalg.norm(gs - gs_h) / np.linalg.norm(gs_h))
    print(f"Tsit5 cylinder N={N} E={E} L=128 mps=15, {K_CYL} save intervals: {K} accepted steps, {st['n_reject']} rejected, "
          f"{st['n_rhs']} RHS; native {t_nat * 1e3:.1f} ms ({t_nat / K * 1e3:.2f} ms/step), host composition {t_host * 1e3:.1f} ms "
          f"({t_host / K * 1e3:.2f} ms/step), x{t_host / t_nat:.2f}; stored {st['stored_bytes']} bytes "
          f"({st['stored_bytes'] / K / 1e3:.1f} KB/step); loss {loss:.6e} vs {loss_h:.6e}, gradient rel L2 {rel:.2e}")
    eng.close()


if TSIT5:
    tsit5_mode()
    sys.exit(0)

pos, cells, ntype, vel = mgn_amd.synth.mesh_cyl(1234, 2000)
eng, onehot, ef, gt, vm, N, E = setup(pos, cells, ntype, vel, K_CYL)
t_nat, (gs, loss) = timed(native(eng, onehot, ef, gt, vm, K_CYL))
host = lambda: ra.solver_training_euler(lambda x: eng.ode_step(x, onehot, ef, vm),
                                        lambda x, lam: eng.ode_vjp(x, onehot, ef, lam, val_mask=vm)[:2], gt[0], gt, DT, vm,
                                        np.full(2, 2.5, np.float32))
t_host, (gs_h, loss_h, _) = timed(host)
rel = float(np.linalg.norm(gs - gs_h) / np.linalg.norm(gs_h))
print(f"cylinder N={N} E={E} L=128 mps=15 K={K_CYL}: native {t_nat * 1e3:.1f} ms ({t_nat / K_CYL * 1e3:.2f} ms/step), "
      f"host composition {t_host * 1e3:.1f} ms ({t_host / K_CYL * 1e3:.2f} ms/step), x{t_host / t_nat:.2f}; "
      f"loss {loss:.6e} vs {loss_h:.6e}, gradient rel L2 {rel:.2e}")
eng.close()

pos, cells = mgn_amd.synth.grid_mesh(500, 250, 1234)
rng = np.random.default_rng(1)
ntype = rng.choice([0, 4, 5, 6], pos.shape[0], p=[0.85, 0.05, 0.05, 0.05]).astype(np.int32)
vel = rng.standard_normal((pos.shape[0], 2)).astype(np.float32)
eng, onehot, ef, gt, vm, N, E = setup(pos, cells, ntype, vel, K_BIG)
t_big, (gs, loss) = timed(native(eng, onehot, ef, gt, vm, K_BIG))
print(f"grid N={N} E={E} L=128 mps=15 K={K_BIG}: native {t_big * 1e3:.1f} ms ({t_big / K_BIG * 1e3:.2f} ms/step), loss {loss:.6e}, "
      f"finite gradient {bool(np.isfinite(gs).all())}")
eng.close()
