"""The in-process transport (MGN_COMM_LOCAL, "local") and the group handle built on it (mgn_group), CPU side: host-only handles
(MGN_DEVICE_NONE) as threads of this process exchange per-node rows along the halo lists by memcpy, reduce in rank order, refuse ids of
the other transports and give up after MGN_COMM_TIMEOUT_S; a host-only group exposes the same partition as ordinary rank handles and
refuses what it must at creation.  Integer-valued rows: every check is exact.  The device side is tests/test_gpu_comm_local.py and
tests/test_gpu_group.py.  Shapes: the small problem of tests/test_gpu_partitioned_step.py (a 40 x 33 grid; P = 2, 3, 4 all have halos)."""
import ctypes as C
import threading
import time

import numpy as np
import pytest

import mgn_amd
from mgn_amd import MGN_DEVICE_NONE, Engine, GroupEngine, MgnError, _capi, synth
from util import cfg_dict, engine_for

NEW_SYMBOLS = ["mgn_group_create", "mgn_group_destroy", "mgn_group_last_error", "mgn_group_rank_handle", "mgn_group_set_params",
               "mgn_group_set_norms", "mgn_group_set_graph", "mgn_group_set_static", "mgn_group_forward", "mgn_group_ode_step",
               "mgn_group_rollout", "mgn_group_step", "mgn_group_latents_randn", "mgn_group_processor_steps_dev",
               "mgn_group_latents_checksum", "mgn_group_synchronize"]


def _mesh():
    pos, cells = synth.grid_mesh(40, 33, 9)
    s, r = synth.cells_to_edges(cells)
    return pos, s, r


def run_ranks(P, body, timeout=60):
    res, errs = {}, {}

    def work(k):
        try:
            res[k] = body(k)
        except BaseException as ex:   # noqa: BLE001
            errs[k] = ex

    ts = [threading.Thread(target=work, args=(k,)) for k in range(P)]
    [t.start() for t in ts]
    [t.join(timeout) for t in ts]
    if errs:
        raise next(iter(errs.values()))
    assert sorted(res) == list(range(P)), "a rank did not finish"
    return [res[k] for k in range(P)]


def test_new_symbols_are_exported_and_bound(lib_built):
    lib = mgn_amd.load()
    assert lib.mgn_abi_version() == 4 == _capi.ABI_VERSION
    assert _capi.MGN_COMM_LOCAL == 2 == mgn_amd.MGN_COMM_LOCAL
    raw = C.CDLL(lib_built)
    for name in NEW_SYMBOLS + ["mgn_debug_comm_a2a"]:
        assert hasattr(raw, name), name
    for name in NEW_SYMBOLS:
        assert name in _capi.PROTOTYPES and getattr(lib, name).argtypes is not None
    assert "mgn_debug_comm_a2a" not in _capi.PROTOTYPES          # a test hook: exported, not declared in the header


@pytest.mark.parametrize("P", [2, 3, 4])
def test_local_transport_host_handles(lib_built, P):
    """halo_exchange_host returns exactly own_rows indexed by halo_nodes; sum and max give the same bits on every rank and equal the
    rank-ordered NumPy sum (values chosen so that the order of a float64 sum shows)."""
    pos, s, r = _mesh()
    cfg = cfg_dict(L=128, mps=3)
    cid = Engine.comm_unique_id("local")
    terms = [np.array([1e16, 1.0, 0.1 * (k + 1)]) * (1.0 if k % 2 == 0 else -1.0) + np.array([0.0, 3.0, 1e-17 * k]) for k in range(P)]

    def body(k):
        e = engine_for(cfg, rank=k, nranks=P, device=MGN_DEVICE_NONE)
        e.set_graph(s, r, pos.shape[0], mesh_pos=pos)
        e.comm_init(cid, "local")
        own, hn = e.owned_nodes(), e.halo_nodes()
        ok = True
        for it, W in enumerate((1, 5, 16)):
            rows = np.stack([(own * (j + 1) + it).astype(np.float32) for j in range(W)], 1)
            want = np.stack([(hn * (j + 1) + it).astype(np.float32) for j in range(W)], 1)
            ok = ok and np.array_equal(e.halo_exchange_host(rows), want)
        tot = e.comm_allreduce(terms[k], "sum")
        mx = e.comm_allreduce(terms[k], "max")
        e.comm_barrier()
        n_halo = e.n_halo
        e.close()
        return ok, tot, mx, n_halo

    res = run_ranks(P, body)
    want_sum = terms[0].copy()
    for t in terms[1:]:
        want_sum = want_sum + t                                   # ascending rank order
    want_max = np.max(np.stack(terms), 0)
    for ok, tot, mx, n_halo in res:
        assert ok and n_halo > 0
        assert tot.tobytes() == want_sum.tobytes() and mx.tobytes() == want_max.tobytes()


def test_file_bootstrap_accepts_the_local_transport(lib_built, tmp_path):
    """mgn_comm_init_file makes and distributes a "local" id like any other (the ranks of one process can do without it; it must not refuse)."""
    pos, s, r = _mesh()
    cfg = cfg_dict(L=128, mps=3)
    path = str(tmp_path / "comm.id")

    def body(k):
        e = engine_for(cfg, rank=k, nranks=2, device=MGN_DEVICE_NONE)
        e.set_graph(s, r, pos.shape[0], mesh_pos=pos)
        e.comm_init_file(path, "local")
        halo = e.halo_exchange_host(e.owned_nodes().astype(np.float32)[:, None])
        ok = np.array_equal(halo[:, 0], e.halo_nodes().astype(np.float32))
        e.comm_barrier()
        e.close()
        return ok

    assert all(run_ranks(2, body))


def test_ids_of_another_transport_are_refused(lib_built):
    for made, used in (("host", "local"), ("local", "host")):
        cid = Engine.comm_unique_id(made)
        e = Engine(9, 3, 2, rank=0, nranks=1, device=MGN_DEVICE_NONE)
        with pytest.raises(MgnError) as ei:
            e.comm_init(cid, used)
        assert ei.value.code == _capi.MGN_E_RCCL and "was not made for" in str(ei.value)
        e.close()


def test_a_missing_peer_is_a_timeout_not_a_hang(lib_built, monkeypatch):
    """Two ranks join; only rank 0 calls the barrier.  With MGN_COMM_TIMEOUT_S = 1 it returns an error within a few seconds and both
    handles can still be destroyed.  (The time limit is read at mgn_comm_init.)"""
    monkeypatch.setenv("MGN_COMM_TIMEOUT_S", "1")
    cid = Engine.comm_unique_id("local")
    joined = threading.Barrier(2)

    def body(k):
        e = Engine(9, 3, 2, rank=k, nranks=2, device=MGN_DEVICE_NONE)
        e.comm_init(cid, "local")
        joined.wait(30)
        out = None
        if k == 0:
            t0 = time.monotonic()
            with pytest.raises(MgnError) as ei:
                e.comm_barrier()
            out = (time.monotonic() - t0, ei.value.code, str(ei.value))
        e.close()
        return out

    took, code, text = run_ranks(2, body)[0]
    assert code == _capi.MGN_E_RCCL and "timed out" in text
    assert 0.9 <= took < 10.0, took


@pytest.mark.parametrize("P", [1, 3])
def test_host_only_group_shows_the_partition_of_rank_handles(lib_built, P):
    pos, s, r = _mesh()
    cfg = cfg_dict(L=128, mps=3)
    N = pos.shape[0]
    with GroupEngine(cfg["Fn"], cfg["Fe"], cfg["O"], cfg["L"], cfg["hidden_layers"], cfg["mps"], devices=[MGN_DEVICE_NONE] * P) as g:
        g.set_graph(s, r, N, mesh_pos=pos)
        for k in range(P):
            view = g.rank_engine(k)
            ref = engine_for(cfg, rank=k, nranks=P, device=MGN_DEVICE_NONE)
            ref.set_graph(s, r, N, mesh_pos=pos)
            assert (view.n_own, view.n_halo, view.e_local) == (ref.n_own, ref.n_halo, ref.e_local)
            assert np.array_equal(view.owned_nodes(), ref.owned_nodes())
            assert np.array_equal(view.halo_nodes(), ref.halo_nodes())
            ref.close()
            view.close()
        for _ in range(2):                                        # compute: no device; the group stays usable (its communicator is rebuilt)
            with pytest.raises(MgnError) as ei:
                g.forward(np.zeros((N, cfg["Fn"]), np.float32), np.zeros((s.size, cfg["Fe"]), np.float32))
            assert ei.value.code == _capi.MGN_E_HIP and "rank" in str(ei.value)
        g.set_graph(s, r, N, mesh_pos=pos)
        assert g.rank_engine(P - 1).n_own > 0
    g.close()                                                      # twice: harmless


def test_group_creation_refusals(lib_built):
    lib = mgn_amd.load()
    cfg = cfg_dict(L=128, mps=3)

    def create(nranks, devices, out=True, **over):
        c = _capi.MgnConfig(cfg["Fn"], cfg["Fe"], cfg["O"], cfg["L"], cfg["hidden_layers"], cfg["mps"], 0, 0, 1, -1, 1, 0, 0, 0)
        for k, v in over.items():
            setattr(c, k, v)
        h = C.c_void_p()
        dev = np.asarray(devices, np.int32) if devices is not None else None
        rc = lib.mgn_group_create(C.byref(c), nranks, _capi.i32(dev), C.byref(h) if out else None)
        if rc == 0:
            lib.mgn_group_destroy(h)
        return rc

    none = MGN_DEVICE_NONE
    assert create(0, [none]) == _capi.MGN_E_ARG
    assert create(65, [none] * 65) == _capi.MGN_E_ARG
    assert create(2, None) == _capi.MGN_E_ARG
    assert create(2, [none, none], out=False) == _capi.MGN_E_ARG
    assert create(2, [none, none], n_edge_sets=2, Fe2=4) == _capi.MGN_E_UNSUPPORTED
    assert "edge sets" in lib.mgn_group_last_error(None).decode()
    assert create(2, [none, none], ln_dims=1) == _capi.MGN_E_UNSUPPORTED
    assert create(1, [none], n_edge_sets=2, Fe2=4) == 0           # single-partition modes stay legal on one rank
    assert create(1, [none], ln_dims=1) == 0
    assert create(64, [none] * 64) == 0
    assert create(2, [none, none], L=48) == _capi.MGN_E_ARG       # whatever mgn_create refuses
    assert "rank 0" in lib.mgn_group_last_error(None).decode()


def _os_threads():
    with open("/proc/self/status") as f:
        return int(next(line for line in f if line.startswith("Threads:")).split()[1])


def test_close_ends_the_worker_threads(lib_built):
    """The workers are the library's own threads: Python's count never sees them, the process's count returns to where it was."""
    py0, os0 = threading.active_count(), _os_threads()
    g = GroupEngine(9, 3, 2, 128, 2, 3, devices=[MGN_DEVICE_NONE] * 3)
    assert _os_threads() == os0 + 3 and threading.active_count() == py0
    g.close()
    g.close()
    assert _os_threads() == os0 and threading.active_count() == py0
