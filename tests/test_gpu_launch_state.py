"""The launch layer's process-wide state (csrc/launch.hpp) under what it was rewritten for: first launches from two host threads at once,
and one process that uses two devices in turn.

The dynamic-LDS grant of a kernel is raised on its first launch, per (device, kernel).  Both cases therefore start where no grant exists:
the first in a fresh child process whose two threads make their first launches together, the second on a device this process has not
launched on yet.  What is compared are bits against an engine that runs alone, and that engine against the float64 oracle with the
bounds of the modules whose cases these are (test_gpu_large_mesh_regimes.py, test_gpu_training_regimes.py); tests/c_abi/launch_state.cpp
checks the book-keeping itself on the host."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch  # noqa: F401  (before the engine's first HIP call)

import test_gpu_large_mesh_regimes as lm
import test_gpu_training_regimes as tr
from util import engine_for, set_num_cus, set_renumber, set_train_f16

pytestmark = pytest.mark.gpu

C8 = 8
# the smallest graph on the 150 KiB ring kernels: 2 C + 1 node tiles and 2 C + 1 edge tiles, each with a last tile of one row
# (families 17 and [11, 10]: k_edge_ring_hs<4>, k_node_ring_hs, k_node_split_h)
N_PROC = E_PROC = lm.rows_of(2 * C8 + 1, 1)
# the smallest input with four-tile streaming blocks: 65 edge tiles, one above 8 per test CU, stream in eight-tile blocks and their factored
# first layer runs launch_lin2 in four-tile blocks over 64 cooperative node tiles
STEP_INPUT = "64 | 65 tiles"
STEP_PLAN = dict(factored0=1, gsets=1, need_gt=1)


def child_main():
    """the body of the child process of test_two_threads_make_their_first_launches_together"""
    s, r, v, e, _, _ = lm.graph(N_PROC, E_PROC)
    d = tr.inputs(STEP_INPUT)
    start = threading.Barrier(2, timeout=120)
    got, errors = [None, None], []

    def worker(k):
        try:
            eng = engine_for(lm.CFG, device=0)
            try:
                start.wait()                                      # no kernel has been launched in this process yet
                eng.set_params(lm.params())
                eng.set_graph(s, r, N_PROC)
                proc = eng.processor_steps(v, e, lm.NSTEPS)
                eng.set_params(d["ps"])
                eng.set_graph(d["s"], d["r"], d["N"])
                got[k] = (proc, eng.step(d["nf"], d["ef"], d["target"], d["mask"]))
            finally:
                eng.close()
        except BaseException as ex:                               # (a thread's exception must fail the child)
            errors.append(ex)
            start.abort()

    with lm.Switches(C8):                                         # test CU count 8, renumbering off
        threads = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    if errors:
        raise errors[0]
    # a third engine, alone, through the checks of the two modules: family codes / regime counts, and the oracle's bounds
    v1, e1, _ = lm.check(N_PROC, E_PROC, C8, 17, lm.NODE_DEFAULT)
    gs1, loss1 = tr.check(STEP_INPUT, C8, "coop", "s8", STEP_PLAN)
    for k in range(2):
        (vk, ek), (gsk, lossk) = got[k]
        assert np.array_equal(vk, v1) and np.array_equal(ek, e1), f"thread {k}: processor_steps differs from the engine that ran alone"
        assert np.array_equal(gsk, gs1) and lossk == loss1, f"thread {k}: step differs from the engine that ran alone"
    assert set_num_cus(0) == 0 and set_renumber(1) == 1 and set_train_f16(1) == 1          # the switches are back
    print("launch_state child OK")


def test_two_threads_make_their_first_launches_together():
    """Two threads, an engine each on device 0, released together into their first launches: processor_steps on the ring kernels (their
    150 KiB grants) and a training step on the streaming kernels (128 KiB).  Both get the bits of a third engine that runs alone
    afterwards, and that one meets TOL_15 / ROW_TOL and the training module's loss and gradient bounds against the float64 oracle."""
    code = "import sys; sys.path[:0] = %r; import test_gpu_launch_state as t; t.child_main()" % [p for p in sys.path if p]
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300,
                         cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert res.returncode == 0 and "launch_state child OK" in res.stdout, res.stdout[-3000:] + res.stderr[-3000:]


def test_two_devices_in_one_process():
    """An engine on device 1 first, closed, then one on device 0, no communicator: a grant made on one device must not stand for the
    other.  Equal bits, and the oracle's bounds."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two visible devices")
    s, r, v, e, rv, re = lm.graph(N_PROC, E_PROC)
    outs = []
    try:
        with lm.Switches(C8):
            for dev in (1, 0):
                eng = engine_for(lm.CFG, device=dev)
                try:
                    eng.set_params(lm.params())
                    eng.set_graph(s, r, N_PROC)
                    outs.append(eng.processor_steps(v, e, lm.NSTEPS))
                finally:
                    eng.close()
    finally:
        torch.cuda.set_device(0)
    (va, ea), (vb, eb) = outs
    assert np.array_equal(va, vb) and np.array_equal(ea, eb)
    assert max(lm.rel_max(va, rv), lm.rel_max(ea, re)) <= lm.TOL_15
    assert max(lm.row_err(va, rv), lm.row_err(ea, re)) <= lm.ROW_TOL
