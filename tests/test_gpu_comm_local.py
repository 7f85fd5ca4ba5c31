"""The in-process transport MGN_COMM_LOCAL ("local") on the device: the ranks are threads that share device 0, rows are pulled out of
the peer's send buffer by k_a2a_pull, and the ranks are ordered by HIP events alone (csrc/comm.cpp, LocalComm).  Reference: the same
thread-ranks over the "host" transport -- unchanged code.  A transport only moves bytes, so every difference is a bug: results are
compared bit for bit; forward and step also meet the float64 oracle.  Run on the MI355X box with `-m gpu`."""
import ctypes as C

import numpy as np
import pytest
import torch

import mgn_amd
from local_case import case, host_ranks, same_bits, thread_ranks
from test_gpu_partitioned_step import TOL_GRAD, TOL_LOSS, check_grads, run_ranks
from util import TOL_15, cfg_dict, engine_for, rel_max

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("P", [2, 3, 4])
def test_local_equals_host_bit_for_bit(P):
    """processor_steps_dev on random latents, forward, step and a 5-step Euler rollout (+ the resident right-hand side): per rank the
    same bits over both transports; what the contract makes global (output, gradient, loss, solution) the same on every rank."""
    c = case()
    host, local = host_ranks(P), thread_ranks(P, "local")
    assert all(n_halo > 0 for _, n_halo, _ in local)
    for (h, _, _), (l, _, _) in zip(host, local):
        same_bits(h, l)
        assert np.array_equal(h["v"], l["v"]) and np.array_equal(h["e"], l["e"]) and h["checksum"] == l["checksum"]
        same_bits(l, local[0][0])
    got = local[0][0]
    assert got["n_rhs"] == 5
    assert rel_max(got["out"], c["ref_out"]) <= TOL_15
    assert abs(got["loss"] - c["ref_loss"]) <= TOL_LOSS * abs(c["ref_loss"])
    check_grads(got["grads"], c["ref_grads"], c["cfg"], TOL_GRAD)
    v = sum(l["v"] for l, _, _ in local)                             # owned rows of every rank: the whole array, each row once
    assert np.all(np.abs(v).sum(1) > 0)


# bytes rank k sends to peer q: 0, 4, 20 and 4108 between different ranks, and to itself
SIZES = [[0, 4, 4108], [20, 4108, 0], [4108, 20, 4]]


def _layout(sizes, residues):
    """offsets with 4 spare bytes between segments; segment q starts at an address = residues[q] mod 16 (4-, not 16-aligned)"""
    off, out = 4, []
    for n, res in zip(sizes, residues):
        while off % 16 != res:
            off += 4
        out.append(off)
        off += n + 4
    return out, off + 12


def test_debug_a2a_unaligned_segments_canary_and_reuse():
    """mgn_debug_comm_a2a at sizes the engine never produces: every received byte is the peer's, nothing outside the segments is touched,
    and three rounds on the same buffers see each round's payload (the peers' reads are ordered before the next overwrite of `send`; the
    two-deep event ring is reused).  Segments from even peers land where source and destination agree mod 16 (vector body with a three-
    dword head), from odd peers where they do not (dword path)."""
    P, ROUNDS = 3, 3
    lib = mgn_amd.load()
    fn = lib.mgn_debug_comm_a2a
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    cfg = cfg_dict(L=128, mps=3)
    cid = mgn_amd.Engine.comm_unique_id("local")
    rng = np.random.default_rng(3)
    plan = []
    for k in range(P):
        sb, rb = SIZES[k], [SIZES[q][k] for q in range(P)]
        so, slen = _layout(sb, [4, 4, 4])
        ro, rlen = _layout(rb, [4, 8, 4])
        assert all(o % 4 == 0 and o % 16 != 0 for o in so + ro)
        plan.append(dict(sb=sb, so=so, slen=slen, rb=rb, ro=ro, rlen=rlen,
                         pay=[rng.integers(0, 256, slen, dtype=np.uint8) for _ in range(ROUNDS)]))

    def body(k):
        p = plan[k]
        e = engine_for(cfg, rank=k, nranks=P, device=0)
        e.comm_init(cid, "local")
        send = torch.zeros(p["slen"], dtype=torch.uint8, device="cuda")
        recv = torch.full((p["rlen"],), 0xA5, dtype=torch.uint8, device="cuda")
        arr = lambda v: (C.c_size_t * P)(*v)   # noqa: E731
        got = []
        for it in range(ROUNDS):
            send.copy_(torch.from_numpy(p["pay"][it]))
            torch.cuda.synchronize()
            rc = fn(e.h, send.data_ptr(), arr(p["sb"]), arr(p["so"]), recv.data_ptr(), arr(p["rb"]), arr(p["ro"]))
            assert rc == 0, lib.mgn_last_error(e.h)
            e.synchronize()
            got.append(recv.cpu().numpy().copy())
        e.comm_barrier()
        e.close()
        return got

    res = run_ranks(P, body)
    for k in range(P):
        p = plan[k]
        for it in range(ROUNDS):
            want = np.full(p["rlen"], 0xA5, np.uint8)
            for q in range(P):
                src = plan[q]["pay"][it][plan[q]["so"][k]:plan[q]["so"][k] + SIZES[q][k]]
                want[p["ro"][q]:p["ro"][q] + p["rb"][q]] = src
            assert np.array_equal(res[k][it], want), (k, it)
