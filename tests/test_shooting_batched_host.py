"""mgn_shooting_grad without a GPU: the binding mirrors against include/mgn_hip.h (the Julia side through tests/test_julia_shim.py's
parsers) and the argument refusals a host-only handle gives before any device work."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import test_julia_shim as js
from mgn_amd import MGN_DEVICE_NONE, Engine, MgnError, _capi, synth
from mgn_amd import reference_api as ra

_CT = {C.c_int32: ("i32", 0), C.c_int64: ("i64", 0), C.POINTER(C.c_int32): ("i32", 1), C.POINTER(C.c_double): ("f64", 1)}


def test_prototype_is_bound(lib_built):
    assert "mgn_shooting_grad" in _capi.PROTOTYPES and hasattr(_capi.load(), "mgn_shooting_grad")
    ret, args = js.c_prototypes()["mgn_shooting_grad"]
    assert ret == ("i32", 0)
    assert args == [("mgn_handle", 1), ("mgn_rollout_desc", 1), ("mgn_shooting_desc", 1), ("f32", 1), ("f32", 1), ("f32", 0),
                    ("f32", 1), ("size", 0), ("f32", 1)]
    assert len(_capi.PROTOTYPES["mgn_shooting_grad"][1]) == len(args)


def test_ctypes_desc_mirror_matches_the_header():
    cf = js.c_struct("mgn_shooting_desc")
    assert [n for n, _ in _capi.MgnShootingDesc._fields_] == [n for n, _ in cf]
    for (n, t), (_, want) in zip(_capi.MgnShootingDesc._fields_, cf):
        assert _CT[t] == want, (n, t, want)


def test_julia_desc_mirror_and_call_match_the_header():
    cf = js.c_struct("mgn_shooting_desc")
    jf = js.julia_struct(os.path.join(js.JULIA_DIR, "MGNHip.jl"), "MgnShootingDesc")
    assert [n for n, _ in jf] == [n for n, _ in cf]
    for (n, jt), (_, ct) in zip(jf, cf):
        assert js._JL[jt] == ct, (n, jt, ct)
    ret, args = js.c_prototypes()["mgn_shooting_grad"]
    text = js._strip_jl_comments(open(os.path.join(js.JULIA_DIR, "MGNHip.jl")).read())
    m = re.search(r"@ccall\s+LIB\.mgn_shooting_grad\(", text)
    assert m
    i, depth = m.end(), 1
    while depth:
        depth += {"(": 1, ")": -1}.get(text[i], 0)
        i += 1
    parts = js._split_top(text[m.end():i - 1])
    rtype = re.match(r"::(\w+)", text[i:]).group(1)
    assert js._compatible(js._JL[rtype], ret)
    assert len(parts) == len(args)
    jl = dict(js._JL, **{"Ref{MgnShootingDesc}": ("mgn_shooting_desc", 1)})
    for k, (a, c) in enumerate(zip(parts, args)):
        t = a.rsplit("::", 1)[1].strip()
        assert js._compatible(jl[t], c), (k, a, c)


def test_windows_of_the_reference():
    # T = 8, interval_size = 4: windows (0, 3), (3, 6), (6, 7) -- the batched route takes exactly these
    assert ra.multiple_shooting_ranges(8, 4) == [(0, 3), (3, 6), (6, 7)]


def test_argument_refusals_host_only(lib_built):
    pos, cells = synth.grid_mesh(4, 3, 1)
    s, r = synth.cells_to_edges(cells)
    N, E = pos.shape[0], s.size
    e = Engine(9, 3, 2, L=32, mps=1, device=MGN_DEVICE_NONE)
    e.set_graph(s, r, N)
    oh = np.zeros((N, 7), np.float32)
    ef = np.zeros((E, 3), np.float32)
    gt = np.zeros((3, N, 2), np.float32)

    def call(windows, **kw):
        W = len(windows)
        return e.shooting_grad(oh, ef, gt, windows, [0.01 * a for a, _ in windows][:W], [0.01 * b for _, b in windows][:W], 0.01, 0.01, **kw)

    cases = [([], {}, _capi.MGN_E_ARG),                                    # W = 0
             ([(1, 1)], {}, _capi.MGN_E_ARG),                              # last <= first
             ([(0, 2), (2, 1)], {}, _capi.MGN_E_ARG),
             ([(1, 3)], {}, _capi.MGN_E_ARG),                              # beyond n_gt
             ([(-1, 1)], {}, _capi.MGN_E_ARG),
             ([(0, 2)], dict(solver="Tsit5", adaptive=True), _capi.MGN_E_UNSUPPORTED),
             ([(0, 2)], {}, _capi.MGN_E_HIP)]                              # well-formed: a host-only handle has no compute path
    for windows, kw, code in cases:
        with pytest.raises(MgnError) as ei:
            call(windows, **kw)
        assert ei.value.code == code, (windows, kw, ei.value)
    e.close()
