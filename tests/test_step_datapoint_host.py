"""Derivative training on a device-resident trajectory, the part that needs no GPU: the six entry points exist and are bound, a
host-only handle refuses them the way it refuses mgn_step, and the NumPy mirror of init_train_step of the derivative strategies
(reference src/strategies.jl:395-416) gives the numbers a hand computation gives."""
import ctypes as C

import numpy as np

import mgn_amd
from mgn_amd import MGN_DEVICE_NONE, Engine, MgnError, synth
from mgn_amd import reference_api as ra

F32 = np.float32
SYMBOLS = ("mgn_train_set_trajectory", "mgn_train_set_noise", "mgn_train_online_norms", "mgn_train_norm_state", "mgn_step_datapoint",
           "mgn_datapoint_export")


def test_symbols_are_exported_and_bound(lib_built):
    lib = mgn_amd.load()
    assert lib.mgn_abi_version() == 4
    raw = C.CDLL(lib_built)
    for name in SYMBOLS:
        assert name in mgn_amd.PROTOTYPES, name
        assert hasattr(raw, name), name
        assert getattr(lib, name).argtypes == mgn_amd.PROTOTYPES[name][1]
    for name in ("set_trajectory", "set_noise", "online_norms", "norm_state", "set_norm_state", "step_datapoint", "datapoint_export"):
        assert callable(getattr(Engine, name))
    assert not hasattr(mgn_amd.engine.GroupEngine, "step_datapoint")


def test_host_only_handle_refuses_like_mgn_step(lib_built):
    e = Engine(5, 3, 2, L=32, mps=2, device=MGN_DEVICE_NONE)
    s, r = synth.random_graph(10, 30, 0)
    e.set_graph(s, r, 10)
    mask = np.arange(10, dtype=np.int32)
    with np.errstate(all="ignore"):
        try:
            e.step(np.zeros((10, 5), F32), np.zeros((30, 3), F32), np.zeros((10, 2), F32), mask)
            want = 0
        except MgnError as ex:
            want = ex.code
    assert want == -2            # MGN_E_HIP: no compute path without a device
    calls = (lambda: e.set_trajectory(np.zeros((3, 10, 2), F32), dt=0.1, node_type_onehot=np.zeros((10, 3), F32), ef_raw=np.zeros((30, 3), F32)),
             lambda: e.set_noise(np.ones(2, F32), np.ones(10, np.uint8), 1),
             lambda: e.set_noise(),
             lambda: e.online_norms(),
             lambda: e.norm_state(0),
             lambda: e.set_norm_state(1, np.zeros(3), np.zeros(3), 0, 0),
             lambda: e.step_datapoint(0, mask),
             lambda: e.datapoint_export(0),
             lambda: e.datapoint_export(0, normalised=False))
    for call in calls:
        try:
            call()
            got = 0
        except MgnError as ex:
            got = ex.code
        assert got == want
    e.set_graph(s, r, 10)          # the handle stays usable


class _Mgn:
    def __init__(self, n_norm, e_norm, o_norm):
        self.n_norm, self.e_norm, self.o_norm = n_norm, e_norm, o_norm


def test_init_train_step_derivative_by_hand():
    # three nodes, one field "velocity" of width 2, two datapoints: the field's frames 0, 1 and the targets' frames 1, 2 (add_targets!)
    raw = np.array([[[1.0, 2.0], [0.5, -1.0], [4.0, 0.0]],
                    [[2.0, 2.5], [0.0, -1.0], [4.0, 3.0]],
                    [[2.0, 6.5], [3.0, -2.0], [1.0, 3.0]]], F32)
    data = {"velocity": raw[:-1], "target|velocity": raw[1:]}
    node_type = ra.one_hot(np.array([0, 1, 0]), 2)
    senders, receivers = np.array([0, 1, 2], np.int32), np.array([1, 2, 0], np.int32)
    ef = np.array([[1.0, 0.0, 1.0], [0.0, 2.0, 2.0], [-1.0, -2.0, 3.0]], F32)
    mgn = _Mgn({"velocity": ra.NormaliserOfflineMeanStd(np.array([1.0, 0.0], F32), np.array([2.0, 4.0], F32)),
                "node_type": ra.NormaliserOfflineMinMax(0.0, 1.0)},
               ra.NormaliserOfflineMeanStd(np.zeros(3, F32), np.array([1.0, 2.0, 4.0], F32)),
               {"velocity": ra.NormaliserOfflineMeanStd(np.array([1.0, -1.0], F32), np.array([2.0, 0.5], F32))})
    args = (["velocity"], ["velocity"], node_type, ef, senders, receivers)
    # scalar dt = 0.5, datapoint 0:  d = (frame 1 - frame 0) / 0.5;  target = (d - mean) / std
    g, tq = ra.init_train_step_derivative(mgn, data, {"dt": 0.5}, *args, 0)
    d0 = np.array([[2.0, 1.0], [-1.0, 0.0], [0.0, 6.0]], F32)
    assert np.array_equal(tq, np.array([[0.5, 4.0], [-1.0, 2.0], [-0.5, 14.0]], F32))
    assert np.array_equal(tq, (d0 - np.array([1.0, -1.0], F32)) / np.array([2.0, 0.5], F32))
    # nf = [(v - mean) / std ; onehot], ef = ef / std, of frame 0
    assert np.array_equal(g.nf, np.array([[0.0, 0.5, 1.0, 0.0], [-0.25, -0.25, 0.0, 1.0], [1.5, 0.0, 1.0, 0.0]], F32))
    assert np.array_equal(g.ef, np.array([[1.0, 0.0, 0.25], [0.0, 1.0, 0.5], [-1.0, -1.0, 0.75]], F32))
    assert g.nf.dtype == F32 and tq.dtype == F32
    # times with unequal steps: datapoint 1 runs from 0.25 to 2.25, a step of 2
    meta = {"dt": np.array([0.0, 0.25, 2.25], F32)}
    g1, tq1 = ra.init_train_step_derivative(mgn, data, meta, *args, 1)
    d1 = np.array([[0.0, 2.0], [1.5, -0.5], [-1.5, 0.0]], F32)               # (frame 2 - frame 1) / 2
    assert np.array_equal(tq1, np.array([[-0.5, 6.0], [0.25, 1.0], [-1.25, 2.0]], F32))
    assert np.array_equal(tq1, (d1 - np.array([1.0, -1.0], F32)) / np.array([2.0, 0.5], F32))
    assert np.array_equal(g1.nf[:, :2], (raw[1] - np.array([1.0, 0.0], F32)) / np.array([2.0, 4.0], F32))
    _, tq0 = ra.init_train_step_derivative(mgn, data, meta, *args, 0)          # the first step is 0.25: four times frame 1 - frame 0
    assert np.array_equal(tq0, ((raw[1] - raw[0]) / F32(0.25) - np.array([1.0, -1.0], F32)) / np.array([2.0, 0.5], F32))
    assert not np.array_equal(tq0, tq)
    # an online output normaliser accumulates the raw change first, then normalises with the renewed statistics
    on = ra.NormaliserOnline(2)
    mgn2 = _Mgn(mgn.n_norm, mgn.e_norm, {"velocity": on})
    _, tq2 = ra.init_train_step_derivative(mgn2, data, {"dt": 0.5}, *args, 0)
    assert on.acc_count == 3 and on.num_accumulations == 1 and np.array_equal(on.acc_sum, d0.sum(0, dtype=np.float64))
    assert np.array_equal(tq2, on.frozen()(d0))
