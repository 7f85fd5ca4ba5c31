"""Shared by tests/test_gpu_comm_local.py and tests/test_gpu_group.py: the small problem of tests/test_gpu_partitioned_step.py (a 40 x 33
grid, L = 128, mps = 3; P = 2, 3, 4 all have halos), one workload over every partitioned entry point, and its run on thread-ranks over the
"host" transport -- unchanged code, computed once per P and shared.  A transport only moves bytes: every other way of running the same P
must give the same bits."""
import functools

import numpy as np

import mgn_amd
import mgn_oracle as orc
from test_gpu_partitioned_step import grid_case, run_ranks
from util import engine_for

DT = 0.01
SEED = 7


@functools.lru_cache(maxsize=None)
def case():
    cfg, pos, s, r, ps, nf, ef, target, mask, ref, ref_loss = grid_case()
    N = pos.shape[0]
    rng = np.random.default_rng(21)
    c = dict(cfg=cfg, pos=pos, s=s, r=r, ps=ps, nf=nf, ef=ef, target=target, mask=mask, ref_grads=ref, ref_loss=ref_loss, N=N,
             x0=rng.standard_normal((N, cfg["O"])).astype(np.float32),
             onehot=orc.one_hot(rng.integers(0, cfg["Fn"] - cfg["O"], N), cfg["Fn"] - cfg["O"], 0).astype(np.float32),
             ef_raw=rng.standard_normal((s.size, cfg["Fe"])).astype(np.float32),
             vm=(rng.random(N) > 0.2).astype(np.float32),
             norms=dict(node=(rng.uniform(0.5, 1.5, cfg["Fn"]), rng.uniform(-0.2, 0.2, cfg["Fn"])),
                        edge=(rng.uniform(0.5, 1.5, cfg["Fe"]), rng.uniform(-0.2, 0.2, cfg["Fe"])),
                        out=(rng.uniform(0.5, 1.5, cfg["O"]), rng.uniform(-0.2, 0.2, cfg["O"]))),
             ref_out=orc.forward(ps, cfg, nf, ef, s, r))
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def setup(e, c):
    e.set_params(c["ps"])
    e.set_norms(**c["norms"])
    e.set_graph(c["s"], c["r"], c["N"], mesh_pos=c["pos"])


def workload(e, c):
    """Every partitioned entry point once, on an Engine (one rank) or a GroupEngine (all of them)."""
    e.latents_randn(SEED)
    e.processor_steps_dev(3)
    got = dict(checksum=e.latents_checksum())
    if hasattr(e, "latents_export"):
        got["v"], got["e"] = e.latents_export()
    got["out"] = e.forward(c["nf"], c["ef"])
    gs, got["loss"] = e.step(c["nf"], c["ef"], c["target"], c["mask"])
    got["grads"] = np.array(gs)
    got["rollout"], st = e.rollout("Euler", c["x0"], c["onehot"], c["ef_raw"], 0.0, 5 * DT, DT, 6, dt=DT, val_mask=c["vm"])
    got["n_rhs"] = st["n_rhs"]
    e.set_static(c["onehot"], c["ef_raw"], c["vm"])
    got["rhs"] = e.ode_step(c["x0"])
    return got


def thread_ranks(P, transport):
    """workload on P rank handles that share device 0, as threads of this process; per rank: (results, n_halo, halo_counts)"""
    c = case()
    cid = mgn_amd.Engine.comm_unique_id(transport) if P > 1 else None

    def body(k):
        e = engine_for(c["cfg"], rank=k, nranks=P, device=0)
        setup(e, c)
        if P > 1:
            e.comm_init(cid, transport)
        got = workload(e, c)
        info = (got, e.n_halo, e.halo_counts())
        if P > 1:
            e.comm_barrier()
        e.close()
        return info

    return run_ranks(P, body)


@functools.lru_cache(maxsize=None)
def host_ranks(P):
    return thread_ranks(P, "host")


def same_bits(a, b, keys=("out", "loss", "grads", "rollout", "rhs", "n_rhs")):
    for k in keys:
        x, y = a[k], b[k]
        assert (np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y), k


def summed_checksum(results):
    """the ranks' latents_checksum added in ascending rank order (what mgn_group_latents_checksum returns)"""
    acc = dict.fromkeys(results[0]["checksum"], 0.0)
    for got in results:
        for k, v in got["checksum"].items():
            acc[k] += v
    return acc
