"""mgn_group / GroupEngine: all P partitions of a mesh driven from one thread (worker threads inside the library, an in-process
communicator).  Reference: P thread-ranks of ordinary handles over the "host" transport (tests/local_case.py), bit for bit; forward and
step also against the float64 oracle.  All ranks share device 0.  Run on the MI355X box with `-m gpu`."""
import threading
import time

import numpy as np
import pytest
import torch   # noqa: F401  (before the engine's first HIP call)

import mgn_amd
import mgn_oracle as orc
from local_case import case, host_ranks, same_bits, setup, summed_checksum, workload
from mgn_amd import GroupEngine, MgnError, _capi
from test_gpu_partitioned_step import TOL_GRAD, TOL_LOSS, check_grads
from util import TOL_15, engine_for, rel_max, scatter_labels

pytestmark = pytest.mark.gpu


def group_for(c, P):
    cfg = c["cfg"]
    return GroupEngine(cfg["Fn"], cfg["Fe"], cfg["O"], cfg["L"], cfg["hidden_layers"], cfg["mps"], devices=[0] * P)


def _os_threads():
    with open("/proc/self/status") as f:
        return int(next(line for line in f if line.startswith("Threads:")).split()[1])


@pytest.mark.parametrize("P", [1, 2, 3])
def test_group_equals_thread_ranks_bit_for_bit(P):
    c = case()
    host = [got for got, _, _ in host_ranks(P)]
    with group_for(c, P) as g:
        setup(g, c)
        got = workload(g, c)
        for k in range(P):
            view = g.rank_engine(k)
            assert (view.n_own > 0) and (view.n_halo > 0) == (P > 1)
    same_bits(got, host[0])
    assert got["checksum"] == summed_checksum(host)
    assert rel_max(got["out"], c["ref_out"]) <= TOL_15
    assert abs(got["loss"] - c["ref_loss"]) <= TOL_LOSS * abs(c["ref_loss"])
    check_grads(got["grads"], c["ref_grads"], c["cfg"], TOL_GRAD)


def test_a_second_trajectory_and_errors_leave_the_group_usable():
    c = case()
    cfg, N = c["cfg"], c["N"]
    nf, ef, target, mask = c["nf"], c["ef"], c["target"], c["mask"]
    with group_for(c, 2) as g:
        setup(g, c)
        gs0, loss0 = g.step(nf, ef, target, mask)
        # the same mesh under scattered labels: a new trajectory on the same group
        pos2, s2, r2, _ = scatter_labels(c["pos"], c["s"], c["r"], seed=4)
        ref2, ref2_loss = orc.step_grads(c["ps"], cfg, nf, ef, s2, r2, target, mask)
        g.set_graph(s2, r2, N, mesh_pos=pos2)
        gs2, loss2 = g.step(nf, ef, target, mask)
        assert abs(loss2 - ref2_loss) <= TOL_LOSS * abs(ref2_loss)
        check_grads(gs2, ref2, cfg, TOL_GRAD)
        # every rank refuses before any collective: the text names a rank, the next step gives the same bits
        bad = mask.copy()
        bad[3] = N + 5
        with pytest.raises(MgnError) as ei:
            g.step(nf, ef, target, bad)
        assert ei.value.code == _capi.MGN_E_ARG and "rank" in str(ei.value)
        gs3, loss3 = g.step(nf, ef, target, mask)
        assert loss3 == loss2 and np.array_equal(gs3, gs2)
        # ONE rank fails while the other is already exchanging: rank 1 loses its communicator behind the group's back.  The group
        # answers with rank 1's own status -- what a bare rank handle without a communicator answers -- far sooner than
        # MGN_COMM_TIMEOUT_S (120 s), and works again at once on a rebuilt communicator
        bare = engine_for(cfg, rank=1, nranks=2, device=0)
        setup(bare, c)
        with pytest.raises(MgnError) as want:
            bare.forward(nf, ef)
        bare.close()
        out0 = g.forward(nf, ef)
        h1 = g.lib.mgn_group_rank_handle(g.g, 1)
        assert g.lib.mgn_comm_destroy(h1) == 0
        t0 = time.monotonic()
        with pytest.raises(MgnError) as ei:
            g.forward(nf, ef)
        took = time.monotonic() - t0
        assert ei.value.code == want.value.code and "rank 1:" in str(ei.value) and "mgn_comm_init" in str(ei.value)
        assert took < 10.0, took
        assert np.array_equal(g.forward(nf, ef), out0)
        gs4, loss4 = g.step(nf, ef, target, mask)
        assert loss4 == loss2 and np.array_equal(gs4, gs2)
    assert abs(loss0 - c["ref_loss"]) <= TOL_LOSS * abs(c["ref_loss"])
    check_grads(gs0, c["ref_grads"], cfg, TOL_GRAD)


def test_graph_network_on_a_group(monkeypatch):
    """GraphNetwork(...; gpus) / MGN_GPUS: the reference-shaped surface (`mgn.model(graph, ps, st)`, `step(mgn, graph, target, mask)`)
    on two partitions gives the group's bits."""
    c = case()
    cfg = c["cfg"]
    host = host_ranks(2)[0][0]
    graph = mgn_amd.FeatureGraph(c["nf"], c["ef"], c["s"], c["r"])
    for how in ("argument", "environment"):
        if how == "environment":
            monkeypatch.setenv("MGN_GPUS", "0,0")
        net = mgn_amd.GraphNetwork(cfg["Fn"], cfg["Fe"] - 1, None, None, None, cfg["O"], cfg["mps"], cfg["L"], cfg["hidden_layers"],
                                   ps=c["ps"], gpus=[0, 0] if how == "argument" else None)
        assert isinstance(net.engine, GroupEngine) and net.engine.nranks == 2
        net.set_graph(c["s"], c["r"], c["N"], mesh_pos=c["pos"])
        out, _ = net.model(graph, net.ps, net.st)
        gs, loss = mgn_amd.step(net, graph, c["target"], c["mask"])
        net.engine.close()
        assert np.array_equal(out, host["out"]) and loss == host["loss"] and np.array_equal(gs, host["grads"])


def test_close_twice_and_no_thread_left():
    c = case()

    def once():
        g = group_for(c, 3)
        setup(g, c)
        g.forward(c["nf"], c["ef"])
        assert threading.active_count() == py0                      # the workers are the library's threads, not Python's
        g.close()
        g.close()

    py0 = threading.active_count()
    once()                                                          # (whatever threads the HIP runtime starts for itself exist now)
    os0 = _os_threads()
    once()
    assert threading.active_count() == py0 and _os_threads() == os0
