"""MGN_SOLVER_TSIT5_FIXED without a GPU: the enum in include/mgn_hip.h and the ABI version it leaves alone, the descriptors Engine.rollout /
rollout_eval build (a recorder in place of the library), reference_api's fixed_step on the stub engine of tests/test_rollout_eval_host.py,
the answer of a host-only handle, and the Julia shim's keyword."""
import inspect
import os
import re

import numpy as np
import pytest

import test_julia_shim as js
from mgn_amd import MGN_DEVICE_NONE, Engine, GroupEngine, MgnError, _capi
from mgn_amd import reference_api as ra
from test_rollout_eval_host import StubEngine, canned, host_engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_names_the_three_solvers_and_keeps_the_abi_version():
    hdr = open(os.path.join(ROOT, "include", "mgn_hip.h")).read()
    m = re.search(r"typedef enum mgn_solver \{([^}]*)\} mgn_solver;", hdr)
    assert m
    names = dict((k.strip(), int(v)) for k, v in (item.split("=") for item in m.group(1).split(",")))
    assert names == {"MGN_SOLVER_EULER": 0, "MGN_SOLVER_TSIT5": 1, "MGN_SOLVER_TSIT5_FIXED": 2}
    assert (_capi.MGN_SOLVER_EULER, _capi.MGN_SOLVER_TSIT5, _capi.MGN_SOLVER_TSIT5_FIXED) == (0, 1, 2)
    assert re.search(r"^#define MGN_ABI_VERSION 4\s*$", hdr, flags=re.M)
    assert _capi.ABI_VERSION == 4
    jl = js._strip_jl_comments(open(os.path.join(js.JULIA_DIR, "MGNHip.jl")).read())
    assert re.search(r"^const ABI_VERSION = 4\b", jl, flags=re.M)
    # no struct moved: the mirrors still match field for field
    cf = js.c_struct("mgn_rollout_desc")
    assert [n for n, _ in _capi.MgnRolloutDesc._fields_] == [n for n, _ in cf]


def test_library_still_reports_abi_version_4(lib_built):
    assert _capi.load().mgn_abi_version() == 4


class RecorderLib:
    """The library with mgn_rollout / mgn_rollout_eval replaced by recorders of the descriptor they are handed."""

    FIELDS = ("solver", "t0", "t1", "dt", "saves_dt", "n_saves", "abstol", "reltol", "inflow_rule", "time_f64", "dt_f64", "n_frames")

    def __init__(self, real):
        self._real, self.calls = real, []

    def _record(self, name, d):
        self.calls.append(dict({f: getattr(d._obj, f) for f in self.FIELDS}, call=name))
        return _capi.MGN_OK

    def mgn_rollout(self, h, d):
        return self._record("mgn_rollout", d)

    def mgn_rollout_eval(self, h, d, e):
        return self._record("mgn_rollout_eval", d)

    def __getattr__(self, name):
        return getattr(self._real, name)


def test_engine_builds_solver_2_only_when_asked(lib_built):
    e, s, r, N, E = host_engine()
    e.set_graph(s, r, N)
    rec = e.lib = RecorderLib(e.lib)
    oh, ef = np.zeros((N, 7), np.float32), np.zeros((E, 3), np.float32)
    gt = np.zeros((3, N, 2), np.float32)
    a = (gt[0], oh, ef)
    grid = (0.0, 0.02, 0.01, 3)

    def last():
        return rec.calls[-1]

    e.rollout("Tsit5", *a, *grid, dt=0.004, adaptive=False)
    assert last()["call"] == "mgn_rollout" and last()["solver"] == 2 and abs(last()["dt"] - 0.004) < 1e-9 and last()["dt_f64"] == 0.004
    e.rollout_eval("Tsit5", *a, gt, *grid, dt=0.004, adaptive=False, time_type=np.float64)
    assert last()["call"] == "mgn_rollout_eval" and last()["solver"] == 2 and last()["time_f64"] == 1
    # the defaults, and Euler whatever `adaptive` says: today's descriptors
    e.rollout("Tsit5", *a, *grid, dt=0.004)
    today = dict(last())
    assert today["solver"] == 1
    e.rollout("Tsit5", *a, *grid, dt=0.004, adaptive=True)
    assert last() == today
    e.rollout("Tsit5", *a, *grid)
    assert last()["solver"] == 1 and last()["dt"] == 0.0
    e.rollout_eval("Tsit5", *a, gt, *grid)
    assert last()["solver"] == 1 and last()["dt"] == 0.0
    for adaptive in (True, False):
        e.rollout("Euler", *a, *grid, dt=0.01, adaptive=adaptive)
        assert last()["solver"] == 0
        e.rollout_eval("Euler", *a, gt, *grid, dt=0.01, adaptive=adaptive)
        assert last()["solver"] == 0
    # a fixed-step call differs from today's in the solver alone
    e.rollout("Tsit5", *a, *grid, dt=0.004, adaptive=False)
    assert {k: v for k, v in last().items() if k != "solver"} == {k: v for k, v in today.items() if k != "solver"}
    e.lib = rec._real
    e.close()
    # the group forms carry the keyword with the same default
    for cls in (Engine, GroupEngine):
        for name in ("rollout", "rollout_eval"):
            assert inspect.signature(getattr(cls, name)).parameters["adaptive"].default is True, (cls, name)


def test_host_only_handle_answers_solver_2_with_e_hip(lib_built):
    e, s, r, N, E = host_engine()
    e.set_graph(s, r, N)
    oh, ef = np.zeros((N, 7), np.float32), np.zeros((E, 3), np.float32)
    gt = np.zeros((3, N, 2), np.float32)
    with pytest.raises(MgnError) as ei:
        e.rollout("Tsit5", gt[0], oh, ef, 0.0, 0.02, 0.01, 3, dt=0.004, adaptive=False)
    assert ei.value.code == _capi.MGN_E_HIP
    with pytest.raises(MgnError) as ei:
        e.rollout_eval("Tsit5", gt[0], oh, ef, gt, 0.0, 0.02, 0.01, 3, dt=0.004, adaptive=False)
    assert ei.value.code == _capi.MGN_E_HIP
    e.close()


def test_reference_api_passes_fixed_step_through_and_keeps_its_defaults():
    gt, pred = canned()
    N = gt.shape[1]
    mask = np.array([1, 2, 4, 8, 11], np.int32)
    stub = StubEngine(pred)
    interval = (0.0, 0.01, 0.04)

    def vs(**kw):
        ra.validation_step(stub, gt, None, None, interval, mask, inflow_mask=np.ones(N), **kw)
        return stub.calls[-1]

    c = vs(solver="Tsit5", solver_dt=0.01, fixed_step=True)
    assert c["adaptive"] is False and c["dt"] == 0.01 and c["solver"] == "Tsit5"
    # the defaults: the call this function has always made (no `adaptive` keyword at all)
    for kw in (dict(solver="Tsit5", solver_dt=0.01), dict(solver="Tsit5"), dict(solver="Tsit5", fixed_step=True),
               dict(solver="Euler", solver_dt=0.01, fixed_step=True), dict(solver="Euler", solver_dt=0.01)):
        assert "adaptive" not in vs(**kw), kw
    assert vs(solver="Tsit5", fixed_step=True)["dt"] == 0.0
    loss_a = ra.validation_step(stub, gt, None, None, interval, mask, solver="Tsit5", solver_dt=0.01)[0]
    loss_b = ra.validation_step(stub, gt, None, None, interval, mask, solver="Tsit5", solver_dt=0.01, fixed_step=True)[0]
    assert loss_a == loss_b                                   # (the stub's canned prediction: the reductions are untouched)

    saves = np.arange(gt.shape[0], dtype=np.float32) * np.float32(0.01)

    def re_(**kw):
        ra.rollout_errors(stub, gt, None, None, 0.0, float(saves[-1]), kw.pop("dt", 0.01), saves, [saves[2]], **kw)
        return stub.calls[-1]

    c = re_(solver="Tsit5", fixed_step=True)
    assert c["adaptive"] is False and c["dt"] == 0.01
    for kw in (dict(solver="Tsit5"), dict(solver="Tsit5", dt=None, fixed_step=True), dict(solver="Euler", fixed_step=True), dict(solver="Euler")):
        assert "adaptive" not in re_(**kw), kw
    for f in (ra.validation_step, ra.rollout_errors):
        assert inspect.signature(f).parameters["fixed_step"].default is False
        assert "src/solve.jl:57-61" in f.__doc__ and "fixed_step=True" in f.__doc__


def test_julia_shim_has_the_keyword_and_the_three_way_solver():
    text = js._strip_jl_comments(open(os.path.join(js.JULIA_DIR, "MGNHip.jl")).read())
    three_way = r"MgnRolloutDesc\(name == :Euler \? 0 : \(fixed_step \? 2 : 1\),"
    assert len(re.findall(three_way, text)) == 2
    assert not re.search(r"MgnRolloutDesc\(name == :Euler \? 0 : 1,", text)
    for fn in ("native_rollout", "rollout_eval", "native_validation_step"):
        m = re.search(r"^function %s\((.*?)\)\n" % fn, text, flags=re.M | re.S)
        assert m and re.search(r"\bfixed_step = false\b", m.group(1)), fn
