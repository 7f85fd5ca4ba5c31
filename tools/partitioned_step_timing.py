"""mgn_step on one slice of the M-1M mesh (L = 128, mps = 15) at nranks = 1 and on P = 2 and P = 4 edge-cut partitions whose ranks are
threads sharing ONE GPU over the MGN_COMM_HOST transport (rows staged through the host).  Per call: the wall time of the slowest rank
(median of the repeats after one warm-up call) and the device memory of one rank: what its first mgn_step allocates -- the training
arena plus, a few tens of MB, the training-order weights, index arrays and exchange buffers; the drop of hipMemGetInfo's free memory
over the ranks' first calls divided by the ranks -- and what its handle holds in all (graph, inference buffers and weights included).
One GPU shared by P ranks cannot show a speed-up: the figures say what the exchange and the finish cost and what a rank holds.

    python3 tools/partitioned_step_timing.py [nx=500] [repeats=3] [ranks=1,2,4]"""
import ctypes as C
import os
import sys
import threading
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch  # noqa: F401  (before the engine's first HIP call)
import mgn_amd
import bench

NX = int(sys.argv[1]) if len(sys.argv) > 1 else 500
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
RANKS = [int(x) for x in (sys.argv[3] if len(sys.argv) > 3 else "1,2,4").split(",")]

pos, s, r = mgn_amd.synth.mesh_1m(1234, NX, NX)
N, E = pos.shape[0], s.size
rng = np.random.default_rng(0)
nf = rng.standard_normal((N, 9)).astype(np.float32)
ef = rng.standard_normal((E, 3)).astype(np.float32)
target = rng.standard_normal((N, 2)).astype(np.float32)
mask = np.sort(rng.choice(N, N // 2, replace=False)).astype(np.int32)
ps = bench.glorot_params()


def run(P):
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    cid = mgn_amd.Engine.comm_unique_id("host") if P > 1 else None
    out, errs = {}, {}
    gate = threading.Barrier(P)

    def body(k):
        try:
            e = mgn_amd.Engine(9, 3, 2, 128, 2, 15, rank=k, nranks=P, device=0)
            e.set_params(ps)
            e.set_graph(s, r, N, mesh_pos=pos)
            if P > 1:
                e.comm_init(cid, "host")
            gate.wait()
            free1 = torch.cuda.mem_get_info()[0] if k == 0 else 0
            gate.wait()
            gs, loss = e.step(nf, ef, target, mask)                # warm-up: weights packed, arena allocated
            gate.wait()
            free2 = torch.cuda.mem_get_info()[0] if k == 0 else 0
            gate.wait()
            e.lib.mgn_debug_train_keep_steps.argtypes = [C.c_void_p]
            kept = e.lib.mgn_debug_train_keep_steps(e.h)
            ts = []
            for _ in range(REPS):
                t = time.perf_counter()
                gs, loss = e.step(nf, ef, target, mask)
                ts.append(time.perf_counter() - t)
            out[k] = (float(np.median(ts)), loss, e.n_own, e.n_halo, e.e_local, (free1 - free2, free0 - free2, kept), gs.copy())
            if P > 1:
                e.comm_barrier()
            e.close()
        except BaseException as ex:   # noqa: BLE001
            errs[k] = ex
            gate.abort()

    th = [threading.Thread(target=body, args=(k,)) for k in range(P)]
    [t.start() for t in th]
    [t.join() for t in th]
    if errs:
        raise next(iter(errs.values()))
    t = max(v[0] for v in out.values())
    first, total, kept = out[0][5]
    print(f"nranks={P}: {t * 1e3:.1f} ms per call; per rank {first / P / 1e9:.3f} GB allocated by the first call (arena), {total / P / 1e9:.3f} GB "
          f"held in all, {kept} of 15 steps stored (rank 0); loss {out[0][1]:.6e}; "
          f"owned / halo rows / local edges per rank: {[(v[2], v[3], v[4]) for _, v in sorted(out.items())]}", flush=True)
    return out[0][6]


print(f"mesh_1m slice {NX} x {NX}: N={N} E={E} L=128 mps=15, mask of {mask.size}", flush=True)
g1 = None
for P in RANKS:
    gp = run(P)
    if P == 1:
        g1 = gp
    elif g1 is not None:
        print(f"  gradient vs nranks=1: relative L2 {np.linalg.norm(gp - g1) / np.linalg.norm(g1):.2e}", flush=True)
