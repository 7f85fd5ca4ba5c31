"""Replica groups and the group forms of Adam and the resident parameters, the part that needs no GPU: the seven symbols are declared,
exported and bound with the header's signatures, the ABI version stands, mgn_group_create_replicas refuses what mgn_group_create
refuses and creates what only a replica group may hold (whole-array LayerNorm, two edge sets), a host-only group answers MGN_E_HIP to
the compute calls and stays usable, and the split rule.  The device side is tests/test_gpu_replica_group.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mgn_amd
from mgn_amd import MGN_DEVICE_NONE, Engine, GroupEngine, MgnError, _capi, synth
import test_julia_shim as js

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mgn_hip.h")
REPLICA_HEADER = os.path.join(ROOT, "include", "mgn_hip_replica.h")
G, I32, I64, SIZE, F32P, I32P, F64P = ("mgn_group", 1), ("i32", 0), ("i64", 0), ("size", 0), ("f32", 1), ("i32", 1), ("f64", 1)
WANT = {
    "mgn_group_create_replicas": [("mgn_config", 1), I32, I32P, ("mgn_group", 2)],
    "mgn_group_step_datapoints": [G, I32P, I32, I32, I32P, I64, I32, F32P, SIZE, F32P, F32P],
    "mgn_group_set_params_dev": [G, F32P, SIZE],
    "mgn_group_get_params_dev": [G, I32, F32P, SIZE],
    "mgn_group_adam_init": [G, ("mgn_adam_desc", 1)],
    "mgn_group_adam_update": [G, F32P, SIZE],
    "mgn_group_adam_state": [G, I32, F32P, F32P, F64P],
}
_CT = {I32: C.c_int32, I64: C.c_int64, SIZE: C.c_size_t, F32P: C.POINTER(C.c_float), I32P: C.POINTER(C.c_int32), F64P: C.POINTER(C.c_double),
       G: C.c_void_p, ("mgn_group", 2): C.POINTER(C.c_void_p), ("mgn_config", 1): C.POINTER(_capi.MgnConfig),
       ("mgn_adam_desc", 1): C.POINTER(_capi.MgnAdamDesc)}


def test_declared_exported_and_bound(lib_built, monkeypatch):
    """The seven are declared in include/mgn_hip_replica.h, the part of the header that mgn_hip.h includes, and bound from
    _capi.REPLICA_PROTOTYPES: the symbol list read from mgn_hip.h itself, and PROTOTYPES with it, stay as the tests of the handle forms
    pin them (no group form of Adam, of set_params_dev or of step_datapoints)."""
    lib = _capi.load()
    raw = C.CDLL(lib_built)
    assert re.search(r'^#include "mgn_hip_replica.h"', open(HEADER).read(), re.M)
    monkeypatch.setattr(js, "HEADER", REPLICA_HEADER)
    protos = js.c_prototypes()
    assert set(protos) == set(WANT) == set(_capi.REPLICA_PROTOTYPES)
    assert not set(WANT) & set(_capi.PROTOTYPES)
    for sym, want in WANT.items():
        assert hasattr(raw, sym), sym
        assert protos[sym] == (("i32", 0), want), sym
        restype, argtypes = _capi.REPLICA_PROTOTYPES[sym]
        assert restype is C.c_int and argtypes == [_CT[a] for a in want], sym
        assert getattr(lib, sym).argtypes == argtypes
    # the handle forms behind the group: the same arguments (mgn_group_get_params_dev adds the rank)
    for sym in ("mgn_group_step_datapoints", "mgn_group_set_params_dev", "mgn_group_adam_init", "mgn_group_adam_update", "mgn_group_adam_state"):
        assert _capi.REPLICA_PROTOTYPES[sym] == _capi.PROTOTYPES[sym.replace("mgn_group_", "mgn_")], sym
    assert _capi.REPLICA_PROTOTYPES["mgn_group_create_replicas"] == _capi.PROTOTYPES["mgn_group_create"]
    with GroupEngine(5, 3, 2, L=32, mps=2, devices=[MGN_DEVICE_NONE], replicas=True) as g:      # (looked up on the instance)
        for name in ("step_datapoints", "set_params_dev", "get_params_dev", "adam_init", "adam_update", "adam_state", "set_adam_state"):
            assert callable(getattr(g, name)), name
    assert not hasattr(raw, "mgn_group_shooting_grad")


def test_the_header_compiles_as_c99_with_its_part(tmp_path):
    """mgn_hip.h with the part it includes is pedantic C99, and the seven prototypes are visible through mgn_hip.h alone"""
    import subprocess
    src = tmp_path / "replica_decl.c"
    src.write_text('#include "mgn_hip.h"\n' + "".join(f"enum {{ n_{s} = sizeof(&{s}) }};\n" for s in WANT) + "int main(void) { return 0; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_abi_version_stands(lib_built):
    lib = _capi.load()
    lib.mgn_abi_version.restype = C.c_int
    assert lib.mgn_abi_version() == 4 == _capi.ABI_VERSION
    assert re.search(r"#define\s+MGN_ABI_VERSION\s+4\b", open(HEADER).read())


def test_the_julia_shim_is_not_extended():
    syms = {c[0] for f in os.listdir(js.JULIA_DIR) if f.endswith(".jl") for c in js.julia_ccalls(os.path.join(js.JULIA_DIR, f))}
    assert not any(s in syms for s in WANT)
    assert "mgn_group_create_replicas" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def _create(lib, n, devices, out=True, cfg=True, **over):
    c = _capi.MgnConfig(5, 3, 2, 32, 2, 2, 0, 0, 1, -1, 1, 0, 0, 0)
    for k, v in over.items():
        setattr(c, k, v)
    h = C.c_void_p()
    dev = np.asarray(devices, np.int32) if devices is not None else None
    rc = lib.mgn_group_create_replicas(C.byref(c) if cfg else None, n, _capi.i32(dev), C.byref(h) if out else None)
    if rc == 0:
        lib.mgn_group_destroy(h)
    return rc


def test_creation_refusals(lib_built):
    lib = mgn_amd.load()
    none = MGN_DEVICE_NONE
    assert _create(lib, 0, [none]) == _capi.MGN_E_ARG
    assert _create(lib, 65, [none] * 65) == _capi.MGN_E_ARG
    assert "1 .. 64" in lib.mgn_group_last_error(None).decode()
    assert _create(lib, 2, None) == _capi.MGN_E_ARG
    assert _create(lib, 2, [none, none], cfg=False) == _capi.MGN_E_ARG
    assert _create(lib, 2, [none, none], out=False) == _capi.MGN_E_ARG
    assert _create(lib, 2, [none, 0]) == _capi.MGN_E_ARG                  # MGN_DEVICE_NONE for some replicas only
    assert _create(lib, 2, [none, -7]) == _capi.MGN_E_ARG
    assert _create(lib, 2, [none, none], L=48) == _capi.MGN_E_ARG         # whatever mgn_create refuses
    assert "replica 0" in lib.mgn_group_last_error(None).decode()
    assert _create(lib, 1, [none]) == 0
    assert _create(lib, 64, [none] * 64) == 0


def test_single_partition_modes_are_created(lib_built):
    """every replica is one partition: what mgn_group_create refuses at nranks > 1 is legal here"""
    lib = mgn_amd.load()
    none = MGN_DEVICE_NONE
    assert _create(lib, 2, [none, none], ln_dims=1) == 0
    assert _create(lib, 2, [none, none], n_edge_sets=2, Fe2=4) == 0
    with GroupEngine(5, 3, 2, L=32, mps=2, devices=[none, none], ln_dims="all", replicas=True) as g:
        view = g.rank_engine(1)
        assert (view.cfg.rank, view.cfg.nranks) == (0, 1)
        view.close()
    with GroupEngine(5, 3, 2, L=32, mps=2, devices=[none, none], Fe2=4, replicas=True) as g:
        assert g.replicas and g.nranks == 2


@pytest.mark.parametrize("P", [1, 2])
def test_host_only_group_answers_e_hip_and_stays_usable(lib_built, P):
    pos, cells = synth.grid_mesh(8, 6, 9)
    s, r = synth.cells_to_edges(cells)
    N = pos.shape[0]
    mask = np.arange(10, dtype=np.int32)
    with GroupEngine(5, 3, 2, L=32, mps=2, devices=[MGN_DEVICE_NONE] * P, replicas=True) as g:
        g.set_graph(s, r, N)
        n = g.param_count
        assert n == Engine(5, 3, 2, L=32, mps=2, device=MGN_DEVICE_NONE).param_count
        zeros = np.zeros(n, F32)
        calls = (lambda: g.step_datapoints((0, 1, 0), mask),
                 lambda: g.step_datapoints((0,), mask, want_grads=False),
                 lambda: g.set_params_dev(zeros),
                 lambda: g.get_params_dev(0),
                 lambda: g.adam_init(),
                 lambda: g.adam_update(),
                 lambda: g.adam_update(zeros),
                 lambda: g.adam_state(),
                 lambda: g.set_adam_state(dict(mt=zeros, vt=zeros, beta_t=np.array([0.9, 0.999]))))
        for i, call in enumerate(calls):
            with pytest.raises(MgnError) as ei:
                call()
            assert ei.value.code == _capi.MGN_E_HIP, (i, str(ei.value))
            with pytest.raises(MgnError) as ei:
                g.get_params_dev(P)
            assert ei.value.code == _capi.MGN_E_ARG
            g.set_graph(s, r, N)                              # the group stays usable: every replica holds the whole mesh
            for k in range(P):
                view = g.rank_engine(k)
                assert view.n_own == N and view.n_halo == 0
                view.close()
        with pytest.raises(MgnError) as ei:                   # the arguments come before the handle's state, as on a handle
            g.step_datapoints([], mask)
        assert ei.value.code == _capi.MGN_E_ARG


def shares(B, P):
    q, r = divmod(B, P)
    return [(k * q + min(k, r), q + (1 if k < r else 0)) for k in range(P)]


def test_the_split_rule():
    """contiguous chunks in listed order, sizes differ by at most one, the larger ones first: at most two sizes per call"""
    for B in range(1, 11):
        for P in range(1, 5):
            sh = shares(B, P)
            assert len(sh) == P and sh[0][0] == 0 and sum(c for _, c in sh) == B
            for (f0, c0), (f1, _) in zip(sh, sh[1:]):
                assert f1 == f0 + c0
            counts = [c for _, c in sh]
            assert counts == sorted(counts, reverse=True) and counts[0] - counts[-1] <= 1
            assert counts[0] == -(-B // P) and len(set(counts)) <= 2
            assert [c for c in counts if c == 0] == [0] * max(0, P - B)
    assert shares(3, 2) == [(0, 2), (2, 1)] and shares(5, 2) == [(0, 3), (3, 2)] and shares(2, 3) == [(0, 1), (1, 1), (2, 0)]
