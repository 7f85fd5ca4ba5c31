"""mgn_step on an edge-cut partitioned mesh (nranks > 1 after mgn_comm_init): every rank passes the GLOBAL arrays and returns the
complete gradient and the loss, the same bits on every rank.  The forward exchanges the owned boundary rows of v once per processor
step; the reverse pass sends the halo rows' gradients back to their owners, which add them in a fixed order.
One-GPU box: the ranks are threads that share device 0 and meet over the MGN_COMM_HOST transport (as in test_gpu_comm.py).
References: the float64 oracle (oracle/mgn_oracle.py step_grads) on the whole mesh and a one-partition engine.
Run on the MI355X box with `-m gpu`."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest
import torch   # before the engine's first HIP call (device-array test), or torch finds no GPU afterwards

import mgn_amd
import mgn_oracle as orc
from mgn_amd import MgnError, _capi, synth
from util import cfg_dict, engine_for, make_params, renumbered, scatter_labels

pytestmark = pytest.mark.gpu

TOL_LOSS = 1e-5      # relative (tests/test_gpu_training_step.py)
TOL_GRAD = 2e-4      # max|d| / max|ref| per parameter tensor
TOL_ORDER = 1e-3     # relative L2 between two summation orders of the same step, and against the oracle above the cooperative range


def check_grads(gs, ref, cfg, tol=TOL_GRAD):
    off, worst = 0, ("", 0.0)
    for bname, tensors in orc.model_layout(cfg["Fn"], cfg["Fe"], cfg["O"], cfg["L"], cfg["hidden_layers"], cfg["mps"]):
        for tname, shape in tensors:
            n = int(np.prod(shape))
            a, b = gs[off:off + n], ref[off:off + n]
            scale = max(np.abs(b).max(), 1e-3 * np.abs(ref).max())
            err = float(np.abs(a - b).max() / scale)
            if err > worst[1]:
                worst = (f"{bname}.{tname}", err)
            off += n
    assert off == ref.size
    assert worst[1] <= tol, worst
    return worst


def problem(cfg, pos, s, r, seed=0, frac=0.6):
    N, E = pos.shape[0], s.size
    rng = np.random.default_rng(seed)
    nf = rng.standard_normal((N, cfg["Fn"])).astype(np.float32)
    ef = rng.standard_normal((E, cfg["Fe"])).astype(np.float32)
    target = rng.standard_normal((N, cfg["O"])).astype(np.float32)
    mask = np.sort(rng.choice(N, max(1, int(frac * N)), replace=False)).astype(np.int32)
    return nf, ef, target, mask


def rel_l2(a, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.linalg.norm(np.asarray(a, np.float64) - ref) / max(np.linalg.norm(ref), 1e-30))


def run_ranks(P, body):
    """body(rank) in P threads (ctypes releases the GIL inside the library); re-raises the first failure."""
    res, errs = {}, {}

    def work(k):
        try:
            res[k] = body(k)
        except BaseException as ex:   # noqa: BLE001
            errs[k] = ex

    ts = [threading.Thread(target=work, args=(k,)) for k in range(P)]
    [t.start() for t in ts]
    [t.join(600) for t in ts]
    if errs:
        raise next(iter(errs.values()))
    assert sorted(res) == list(range(P)), "a rank did not finish"
    return [res[k] for k in range(P)]


def partitioned_steps(cfg, ps, pos, s, r, P, calls, info=None):
    """P ranks over the host transport; calls: [(nf, ef, target, mask, mask_index_base, out)], made in order by every rank.
    Returns per rank ([(grads as a host array, loss)], n_halo, info(engine))."""
    cid = mgn_amd.Engine.comm_unique_id("host")
    N = pos.shape[0]

    def body(k):
        e = engine_for(cfg, rank=k, nranks=P, device=0)
        e.set_params(ps)
        e.set_graph(s, r, N, mesh_pos=pos)
        e.comm_init(cid, "host")
        got = []
        for nf, ef, target, mask, base, out in calls:
            gs, loss = e.step(nf, ef, target, mask, mask_index_base=base, out=out(k) if out else None)
            got.append((gs.cpu().numpy().copy() if hasattr(gs, "cpu") else gs.copy(), loss))
        extra = info(e) if info else None
        n_halo = e.n_halo
        e.comm_barrier()
        e.close()
        return got, n_halo, extra

    return run_ranks(P, body)


def single_step(cfg, ps, s, r, N, nf, ef, target, mask):
    eng = engine_for(cfg)
    eng.set_params(ps)
    eng.set_graph(s, r, N)
    res = eng.step(nf, ef, target, mask)
    eng.close()
    return res


def assert_same_bits(results):
    """every rank, every call: the gradient and loss of rank 0's first call, bit for bit"""
    g0, l0 = results[0][0][0]
    for got, _, _ in results:
        for gs, loss in got:
            assert loss == l0 and np.array_equal(gs, g0)
    return g0, l0


# ---- the shared small problem: a 40 x 33 grid, cooperative kernels ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def grid_case(L=128, mps=3, hidden_layers=2):
    cfg = cfg_dict(L=L, mps=mps)
    cfg["hidden_layers"] = hidden_layers
    pos, cells = synth.grid_mesh(40, 33, 9)
    s, r = synth.cells_to_edges(cells)
    ps = make_params(cfg).astype(np.float32)
    nf, ef, target, mask = problem(cfg, pos, s, r)
    ref, ref_loss = orc.step_grads(ps, cfg, nf, ef, s, r, target, mask)
    for a in (pos, s, r, ps, nf, ef, target, mask, ref):
        a.setflags(write=False)
    return cfg, pos, s, r, ps, nf, ef, target, mask, ref, ref_loss


def check_against_oracle(cfg, gs, loss, ref, ref_loss):
    assert abs(loss - ref_loss) <= TOL_LOSS * abs(ref_loss), (loss, ref_loss)
    check_grads(gs, ref, cfg)


@pytest.mark.parametrize("P,L,hidden_layers", [(2, 128, 2), (3, 128, 2), (2, 32, 3)])
def test_partitioned_step_small_mesh(P, L, hidden_layers):
    """Loss and gradient on P partitions: the same bits on every rank and on a second call, the oracle's within the tolerances of the
    one-partition step, a one-partition engine's within the bound between two summation orders."""
    cfg, pos, s, r, ps, nf, ef, target, mask, ref, ref_loss = grid_case(L, 3, hidden_layers)
    res = partitioned_steps(cfg, ps, pos, s, r, P, [(nf, ef, target, mask, 0, None)] * 2)
    assert all(n_halo > 0 for _, n_halo, _ in res)
    gs, loss = assert_same_bits(res)
    check_against_oracle(cfg, gs, loss, ref, ref_loss)
    g1, l1 = single_step(cfg, ps, s, r, pos.shape[0], nf, ef, target, mask)
    assert abs(loss - l1) <= TOL_LOSS * abs(l1)
    assert rel_l2(gs, g1) <= TOL_ORDER


@pytest.mark.parametrize("which", ["rank0", "boundary"])
def test_gradient_reaches_a_rank_that_owns_no_mask_entry(which):
    """P = 2.  rank0: the mask lists only nodes rank 0 owns -- rank 1 owns no entry, its loss term is empty, and everything its edges and
    nodes contribute to the gradient arrives through the reverse exchange.  boundary: only nodes that some peer lists as halo."""
    cfg, pos, s, r, ps, nf, ef, target, _, _, _ = grid_case()
    N = pos.shape[0]
    owner = mgn_amd.Engine.partition_nodes(N, 2, mesh_pos=pos)
    if which == "rank0":
        mask = np.nonzero(owner == 0)[0][::2].astype(np.int32)
        assert mask.size > 0 and not np.any(owner[mask] == 1)
    else:
        halos = partitioned_halo_nodes(cfg, pos, s, r, 2)
        mask = np.unique(np.concatenate(halos)).astype(np.int32)
        assert set(owner[mask]) == {0, 1}
    ref, ref_loss = orc.step_grads(ps, cfg, nf, ef, s, r, target, mask)
    if which == "rank0":   # not vacuous: without the edges that rank 1 holds (receiver-owned) the gradient is another one
        keep = owner[r] != 1
        cut, _ = orc.step_grads(ps, cfg, nf, ef[keep], s[keep], r[keep], target, mask)
        assert rel_l2(cut, ref) > 10 * TOL_GRAD
    res = partitioned_steps(cfg, ps, pos, s, r, 2, [(nf, ef, target, mask, 0, None)], info=lambda e: e.node_owner())
    assert all(np.array_equal(o, owner) for _, _, o in res)
    gs, loss = assert_same_bits(res)
    check_against_oracle(cfg, gs, loss, ref, ref_loss)


def partitioned_halo_nodes(cfg, pos, s, r, P):
    """global ids of every rank's halo nodes (host-only handles: the partition is a host computation)"""
    out = []
    for k in range(P):
        e = engine_for(cfg, rank=k, nranks=P, device=_capi.MGN_DEVICE_NONE)
        e.set_graph(s, r, pos.shape[0], mesh_pos=pos)
        out.append(e.halo_nodes())
        e.close()
    return out


def test_a_node_that_is_halo_to_two_peers():
    """P = 4: where the cuts of the bisection meet, an owned row is sent to two peers and receives two halo gradients, added in rank order."""
    cfg, pos, s, r, ps, nf, ef, target, mask, ref, ref_loss = grid_case()

    def info(e):
        counts, _ = e.halo_counts()
        idx = e.halo_send_index()
        lists = np.split(idx, np.cumsum(counts)[:-1])
        assert all(np.unique(li).size == li.size for li in lists)          # (a peer lists a row once)
        return int((np.unique(idx, return_counts=True)[1] >= 2).sum()) if idx.size else 0

    res = partitioned_steps(cfg, ps, pos, s, r, 4, [(nf, ef, target, mask, 0, None)] * 2, info=info)
    assert all(n_halo > 0 for _, n_halo, _ in res)
    assert any(shared > 0 for _, _, shared in res), "no owned row is in two peers' send lists"
    gs, loss = assert_same_bits(res)
    check_against_oracle(cfg, gs, loss, ref, ref_loss)


def test_streaming_kernels_and_factored_first_layer(monkeypatch):
    """Two partitions of a 149 x 149 slice of the M-1M mesh, the smallest whose local edge lists both exceed 2048 tiles: streaming edge
    kernels, factored first layer (P / Q over owned + halo rows, dW1_sender over all local rows), stored and recomputed steps."""
    cfg = cfg_dict(L=128, mps=2)
    pos, s, r = synth.mesh_1m(7, 149, 149)
    N = pos.shape[0]
    ps = make_params(cfg).astype(np.float32)
    nf, ef, target, mask = problem(cfg, pos, s, r, seed=5, frac=0.3)
    calls = [(nf, ef, target, mask, 0, None)] * 2
    def info(e):
        e.lib.mgn_debug_train_keep_steps.argtypes = [C.c_void_p]
        return e.e_local, e.lib.mgn_debug_train_keep_steps(e.h)

    res = partitioned_steps(cfg, ps, pos, s, r, 2, calls, info=info)
    assert all(x[0] > 2048 * 32 for _, _, x in res), [x[2] for x in res]
    assert all(x[1] == cfg["mps"] for _, _, x in res)                      # every step's activations stored
    assert all(n_halo > 0 for _, n_halo, _ in res)
    gs, loss = assert_same_bits(res)
    ref, ref_loss = orc.step_grads(ps, cfg, nf, ef, s, r, target, mask)
    assert abs(loss - ref_loss) <= TOL_LOSS * abs(ref_loss), (loss, ref_loss)
    assert rel_l2(gs, ref) <= TOL_ORDER
    monkeypatch.setenv("MGN_TRAIN_KEEP_STEPS", "0")                        # every processor step recomputed in the reverse pass
    res0 = partitioned_steps(cfg, ps, pos, s, r, 2, calls[:1], info=info)
    assert all(x[1] == 0 for _, _, x in res0)                              # ... and none: the handles did recompute
    g0, l0 = assert_same_bits(res0)
    assert l0 == loss
    assert rel_l2(g0, gs) <= TOL_ORDER


def test_scattered_labels_device_arrays_and_one_based_mask():
    """The mesh under arbitrary node labels (the engine renumbers its rows), inputs and the gradient as device tensors, and the mask
    1-based as at the Julia boundary: the same bits as 0-based."""
    cfg, pos0, s0, r0, ps, nf, ef, target, mask, _, _ = grid_case()
    pos, s, r, _ = scatter_labels(pos0, s0, r0, seed=4)
    ref, ref_loss = orc.step_grads(ps, cfg, nf, ef, s, r, target, mask)
    dev = torch.device("cuda")
    d_nf, d_ef, d_t = (torch.from_numpy(np.array(a)).to(dev) for a in (nf, ef, target))
    outs = [torch.zeros(ref.size, dtype=torch.float32, device=dev) for _ in range(2)]
    calls = [(d_nf, d_ef, d_t, mask, 0, lambda k: outs[k]), (nf, ef, target, mask + 1, 1, None)]
    res = partitioned_steps(cfg, ps, pos, s, r, 2, calls, info=renumbered)
    assert all(n_halo > 0 for _, n_halo, _ in res)
    assert any(rn for _, _, rn in res), "the scattered labels did not make the engine renumber"
    gs, loss = assert_same_bits(res)
    check_against_oracle(cfg, gs, loss, ref, ref_loss)


def test_refusals_leave_the_handle_usable():
    cfg, pos, s, r, ps, nf, ef, target, mask, ref, ref_loss = grid_case()
    N = pos.shape[0]
    cid = mgn_amd.Engine.comm_unique_id("host")
    solver_args = (np.zeros((N, 2), np.float32), np.zeros((N, 7), np.float32), np.zeros((s.size, 3), np.float32),
                   np.zeros((3, N, 2), np.float32), 0.0, 0.02, 0.01, 0.01, 3)

    def body(k):
        e = engine_for(cfg, rank=k, nranks=2, device=0)
        e.set_params(ps)
        e.set_graph(s, r, N, mesh_pos=pos)
        with pytest.raises(MgnError) as ei:                                # no communicator yet
            e.step(nf, ef, target, mask)
        assert ei.value.code == _capi.MGN_E_STATE and "mgn_comm_init" in str(ei.value)
        e.comm_init(cid, "host")
        first = e.step(nf, ef, target, mask)
        gbuf, loss = np.zeros(e.param_count, np.float32), C.c_float()      # grads of the wrong size: refused before any collective
        rc = e.lib.mgn_step(e.h, _capi.f32(np.array(nf)), _capi.f32(np.array(ef)), _capi.f32(np.array(target)), _capi.i32(np.array(mask)),
                            mask.size, 0, _capi.f32(gbuf), e.param_count - 1, C.byref(loss))
        assert rc == _capi.MGN_E_ARG
        again = e.step(nf, ef, target, mask)
        with pytest.raises(MgnError) as ei:
            e.solver_grad(*solver_args)
        assert ei.value.code == _capi.MGN_E_STATE and "partition" in str(ei.value)
        last = e.step(nf, ef, target, mask)
        e.comm_barrier()
        e.close()
        return [first, again, last]

    res = run_ranks(2, body)
    g0, l0 = res[0][0]
    for got in res:
        for gs, loss in got:
            assert loss == l0 and np.array_equal(gs, g0)
    check_against_oracle(cfg, g0, l0, ref, ref_loss)
    # two edge sets on a partitioned handle with its communicator: refused on every rank, nobody waits for a peer.  (No valid step exists
    # on such a handle; it still answers and still meets its peers.)
    cid2 = mgn_amd.Engine.comm_unique_id("host")

    def body2(k):
        two = mgn_amd.Engine(cfg["Fn"], cfg["Fe"], cfg["O"], cfg["L"], 2, cfg["mps"], rank=k, nranks=2, device=0, Fe2=4)
        two.set_params(np.zeros(two.param_count, np.float32))
        two.set_graph(s, r, N, mesh_pos=pos)
        two.comm_init(cid2, "host")
        with pytest.raises(MgnError) as ei:
            two.step(nf, ef, target, mask)
        assert ei.value.code == _capi.MGN_E_UNSUPPORTED
        assert two.n_halo > 0 and two.halo_nodes().size == two.n_halo
        two.comm_barrier()
        two.close()
        return True

    assert all(run_ranks(2, body2))
