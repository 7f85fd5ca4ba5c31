"""Derivative training on partitions, the part that needs no GPU: the group's six datapoint calls exist, are declared and bound; a
host-only group refuses them as it refuses every compute call and stays usable; and the rank-ordered sum of the online normalisers
(per-rank partial sums over the partition's owner map, added in ascending rank order in double) stays within the worst-case bound of a
double summation from NumPy's float64 sums.  The device side is tests/test_gpu_group_datapoint.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mgn_amd
from mgn_amd import MGN_DEVICE_NONE, Engine, GroupEngine, MgnError, _capi, synth

F32 = np.float32
SYMBOLS = ("mgn_group_train_set_trajectory", "mgn_group_train_set_noise", "mgn_group_train_online_norms", "mgn_group_train_norm_state",
           "mgn_group_step_datapoint", "mgn_group_datapoint_export")
METHODS = ("set_trajectory", "set_noise", "online_norms", "norm_state", "set_norm_state", "step_datapoint", "datapoint_export")


def _mesh():
    pos, cells = synth.grid_mesh(40, 33, 9)
    s, r = synth.cells_to_edges(cells)
    return pos, s, r


def test_symbols_are_exported_declared_and_bound(lib_built):
    lib = mgn_amd.load()
    assert lib.mgn_abi_version() == 4 == _capi.ABI_VERSION          # symbols were added; no struct or prototype changed
    raw = C.CDLL(lib_built)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "mgn_hip.h")).read()
    declared = set(re.findall(r"\bint (mgn_[a-z0-9_]+)\s*\(", hdr))
    for name in SYMBOLS:
        assert hasattr(raw, name), name
        assert name in declared, name
        assert name in _capi.PROTOTYPES, name
        # the arguments of the rank handle's call of the same name behind the handle
        assert _capi.PROTOTYPES[name] == _capi.PROTOTYPES[name.replace("mgn_group_", "mgn_")], name
        assert getattr(lib, name).argtypes == _capi.PROTOTYPES[name][1]
    with GroupEngine(5, 3, 2, L=32, mps=2, devices=[MGN_DEVICE_NONE]) as g:      # (step_datapoint is looked up on the instance)
        for name in METHODS:
            assert callable(getattr(g, name)) and callable(getattr(Engine, name)), name


@pytest.mark.parametrize("P", [1, 2])
def test_host_only_group_answers_e_hip_and_stays_usable(lib_built, P):
    pos, s, r = _mesh()
    N, E = pos.shape[0], s.size
    mask = np.arange(10, dtype=np.int32)
    with GroupEngine(5, 3, 2, L=32, mps=2, devices=[MGN_DEVICE_NONE] * P) as g:
        g.set_graph(s, r, N, mesh_pos=pos)
        kw = dict(dt=0.1, node_type_onehot=np.zeros((N, 3), F32), ef_raw=np.zeros((E, 3), F32))
        calls = (lambda: g.set_trajectory(np.zeros((3, N, 2), F32), **kw),
                 lambda: g.set_noise(np.ones(2, F32), np.ones(N, np.uint8), 1),
                 lambda: g.set_noise(),
                 lambda: g.online_norms(),
                 lambda: g.norm_state(0),
                 lambda: g.set_norm_state(1, np.zeros(3), np.zeros(3), 0, 0),
                 lambda: g.step_datapoint(0, mask),
                 lambda: g.datapoint_export(0),
                 lambda: g.datapoint_export(0, normalised=False))
        for i, call in enumerate(calls):
            with pytest.raises(MgnError) as ei:
                call()
            assert ei.value.code == _capi.MGN_E_HIP, (i, str(ei.value))
            assert "rank" in str(ei.value)
            g.set_graph(s, r, N, mesh_pos=pos)              # the group stays usable: the partition is rebuilt, the ranks answer
            assert sum(g.rank_engine(k).n_own for k in range(P)) == N


@pytest.mark.parametrize("P", [2, 3, 4])
def test_rank_ordered_totals_stay_within_the_summation_bound(lib_built, P):
    """What an accumulating step adds on P ranks, mirrored in NumPy: every rank's column sums and sums of squares over the rows it owns
    (mgn_partition_nodes' owner map), the ranks' parts added in ascending rank order.  Against np.sum in float64 the difference stays
    within rows * 2^-52 * sum |x| (sum x^2 for the squares), the worst case of a double summation in any order; the order of the ranks
    is what fixes the bits, so another order may differ from it but stays within the same bound."""
    pos, _, _ = _mesh()
    N = pos.shape[0]
    owner = Engine.partition_nodes(N, P, mesh_pos=pos)
    assert sorted(set(owner)) == list(range(P))
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((N, 2)) * np.array([1.5, 300.0]) + np.array([2.0, -50.0])).astype(F32).astype(np.float64)

    def rank_ordered(order):
        s, q = np.zeros(2), np.zeros(2)
        for k in order:
            rows = x[owner == k]
            ps, pq = np.zeros(2), np.zeros(2)
            for row in rows:                                # a plain running sum: no pairwise trick hides the order
                ps += row
                pq += row * row
            s, q = s + ps, q + pq
        return s, q

    s, q = rank_ordered(range(P))
    bound_s, bound_q = N * 2.0 ** -52 * np.abs(x).sum(0), N * 2.0 ** -52 * (x * x).sum(0)
    assert np.all(np.abs(s - x.sum(0)) <= bound_s) and np.all(np.abs(q - (x * x).sum(0)) <= bound_q)
    s2, q2 = rank_ordered(range(P))
    assert np.array_equal(s, s2) and np.array_equal(q, q2)                  # repeatable for a partition
    s3, q3 = rank_ordered(reversed(range(P)))
    assert np.all(np.abs(s3 - s) <= 2 * bound_s) and np.all(np.abs(q3 - q) <= 2 * bound_q)
