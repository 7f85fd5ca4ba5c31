"""mgn_rollout_eval without a GPU: the binding mirrors against include/mgn_hip.h (the Julia side through tests/test_julia_shim.py's
parsers), reference_api.validation_step / rollout_errors on a stub engine against a direct NumPy transcription of the reference's
lines (src/strategies.jl:123-133, src/MeshGraphNets.jl:615-628), and the refusals a host-only handle gives before any device work."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import test_julia_shim as js
from mgn_amd import MGN_DEVICE_NONE, Engine, MgnError, _capi, synth
from mgn_amd import reference_api as ra

_CT = {C.c_int32: ("i32", 0), C.c_int64: ("i64", 0), C.c_double: ("f64", 0), C.POINTER(C.c_int32): ("i32", 1),
       C.POINTER(C.c_double): ("f64", 1), C.POINTER(C.c_float): ("f32", 1)}


def test_symbol_is_exported_and_bound(lib_built):
    assert "mgn_rollout_eval" in _capi.PROTOTYPES and hasattr(_capi.load(), "mgn_rollout_eval")
    ret, args = js.c_prototypes()["mgn_rollout_eval"]
    assert ret == ("i32", 0)
    assert args == [("mgn_handle", 1), ("mgn_rollout_desc", 1), ("mgn_rollout_eval_desc", 1)]
    assert len(_capi.PROTOTYPES["mgn_rollout_eval"][1]) == len(args)
    assert _capi.load().mgn_abi_version() == 4       # a new symbol only


def test_ctypes_desc_mirror_matches_the_header():
    cf = js.c_struct("mgn_rollout_eval_desc")
    assert [n for n, _ in cf] == ["gt", "n_gt", "mse_save", "mse_time", "sel", "n_sel", "sel_index_base", "val_loss"]
    assert [n for n, _ in _capi.MgnRolloutEvalDesc._fields_] == [n for n, _ in cf]
    for (n, t), (_, want) in zip(_capi.MgnRolloutEvalDesc._fields_, cf):
        assert _CT[t] == want, (n, t, want)


def test_julia_desc_mirror_and_call_match_the_header():
    cf = js.c_struct("mgn_rollout_eval_desc")
    jf = js.julia_struct(os.path.join(js.JULIA_DIR, "MGNHip.jl"), "MgnRolloutEvalDesc")
    assert [n for n, _ in jf] == [n for n, _ in cf]
    for (n, jt), (_, ct) in zip(jf, cf):
        assert js._JL[jt] == ct, (n, jt, ct)
    ret, args = js.c_prototypes()["mgn_rollout_eval"]
    text = js._strip_jl_comments(open(os.path.join(js.JULIA_DIR, "MGNHip.jl")).read())
    m = re.search(r"@ccall\s+LIB\.mgn_rollout_eval\(", text)
    assert m
    i, depth = m.end(), 1
    while depth:
        depth += {"(": 1, ")": -1}.get(text[i], 0)
        i += 1
    parts = js._split_top(text[m.end():i - 1])
    assert js._compatible(js._JL[re.match(r"::(\w+)", text[i:]).group(1)], ret)
    assert len(parts) == len(args)
    jl = dict(js._JL, **{"Ref{MgnRolloutEvalDesc}": ("mgn_rollout_eval_desc", 1)})
    for k, (a, c) in enumerate(zip(parts, args)):
        assert js._compatible(jl[a.rsplit("::", 1)[1].strip()], c), (k, a, c)
    for name in ("rollout_eval", "native_validation_step"):
        assert re.search(r"export[^\n]*\b%s\b" % name, text) and re.search(r"^function %s\(" % name, text, flags=re.M)


# ---- reference_api on a stub engine ---------------------------------------------------------------------------------------------------
class StubEngine:
    """Engine.rollout_eval's contract in NumPy over a canned prediction (linear `sel`, float64 sums); records what it was called with."""

    def __init__(self, pred):
        self.pred = pred
        self.calls = []

    def rollout_eval(self, solver, x0, node_type_onehot, ef_raw, gt, t0, t1, saves_dt, n_saves, sel=None, sel_index_base=0, want_pred=False,
                     **kw):
        self.calls.append(dict(kw, solver=solver, x0=x0, gt=gt, t0=t0, t1=t1, saves_dt=saves_dt, n_saves=n_saves, sel=sel,
                               sel_index_base=sel_index_base, want_pred=want_pred))
        pred = self.pred[:n_saves]
        q = (pred.astype(np.float64) - np.asarray(gt[:n_saves], np.float64)) ** 2
        mse_time = q.mean(axis=0)
        flat = mse_time.reshape(-1)
        val = flat.mean() if sel is None or len(sel) == 0 else flat[np.asarray(sel, np.int64) - sel_index_base].mean()
        return {"val_loss": float(val), "mse_save": q.mean(axis=1), "mse_time": mse_time.astype(np.float32), "pred": pred if want_pred else None,
                "stats": dict(n_accept=0, n_reject=0, n_rhs=0)}


def canned(T=7, N=12, O=2, seed=4):
    rng = np.random.default_rng(seed)
    gt = rng.standard_normal((T, N, O)).astype(np.float32)
    pred = (gt + 0.1 * rng.standard_normal((T, N, O)) * (1 + np.arange(T))[:, None, None]).astype(np.float32)
    return gt, pred


def julia(a):
    """[count][N][O] -> the reference's O x N x count array."""
    return np.transpose(a, (2, 1, 0))


def test_validation_step_is_the_references_lines_with_linear_indexing():
    gt, pred = canned()
    N, O = gt.shape[1:]
    mask1 = np.array([2, 3, 5, 9, 12], np.int32)            # 1-based node indices, as `findall` gives them
    stub = StubEngine(pred)
    n_saves = 5
    loss, g, p = ra.validation_step(stub, gt, None, None, (0.0, 0.01, 0.04), mask1, solver="Euler", solver_dt=0.01, inflow_mask=np.ones(N),
                                    mask_index_base=1, want_arrays=True)
    # strategies.jl:123-133, transcribed: gt / prediction are O x N x T, error = mean(.^2; dims = 3), mean(error[mask]) -- a vector
    # of integers indexing a matrix is LINEAR (column-major) indexing
    jgt, jpred = julia(gt)[:, :, :n_saves], julia(pred)[:, :, :n_saves]
    error = ((jpred.astype(np.float64) - jgt) ** 2).mean(axis=2)
    want = error.reshape(-1, order="F")[mask1 - 1].mean()
    assert abs(loss - want) <= 1e-15 * want
    whole_nodes = error[:, mask1 - 1].mean()
    assert abs(want - whole_nodes) > 1e-3 * whole_nodes       # O = 2: "nodes" and "linear" are different numbers; linear is asserted
    assert np.array_equal(g, gt[:n_saves]) and np.array_equal(p, pred[:n_saves])
    c = stub.calls[-1]
    assert c["n_saves"] == n_saves and c["t0"] == 0.0 and abs(c["t1"] - 0.04) < 1e-6 and c["saves_dt"] == 0.01 and c["dt"] == 0.01
    assert c["gt"] is gt and c["inflow_data"] is gt           # one array object: one pointer at the C call
    assert np.array_equal(c["x0"], gt[0]) and c["sel_index_base"] == 1
    loss0, g0, p0 = ra.validation_step(stub, gt, None, None, (0.0, 0.01, 0.04), mask1 - 1, solver="Tsit5")
    assert loss0 == loss and g0 is None and p0 is None
    assert stub.calls[-1]["inflow_data"] is None and stub.calls[-1]["dt"] == 0.0 and not stub.calls[-1]["want_pred"]
    with pytest.raises(ValueError):
        ra.validation_step(stub, gt[:3], None, None, (0.0, 0.01, 0.04), mask1 - 1)


def test_rollout_errors_is_eval_networks_table():
    gt, pred = canned()
    T = gt.shape[0]
    saves = np.arange(T, dtype=np.float32) * np.float32(0.01)
    horizons = [saves[1], saves[4], saves[T - 1]]
    stub = StubEngine(pred)
    error, table = ra.rollout_errors(stub, gt, None, None, 0.0, float(saves[-1]), 0.01, saves, horizons, solver="Euler")
    # MeshGraphNets.jl:615-628, transcribed: error = mean((prediction - gt) .^ 2; dims = 2) is O x 1 x T
    jerr = ((julia(pred).astype(np.float64) - julia(gt)) ** 2).mean(axis=1, keepdims=True)
    assert np.allclose(error, jerr[:, 0, :].T, rtol=1e-15, atol=0)
    for hz in horizons:
        k = int(np.nonzero(saves == hz)[0][0])
        err, cum = jerr[:, 0, k].mean(), jerr[:, 0, :k + 1].mean()
        got = table[hz]
        assert abs(got[0] - err) <= 1e-14 * err and abs(got[1] - cum) <= 1e-14 * cum and abs(got[2] - np.sqrt(cum)) <= 1e-14 * np.sqrt(cum)
    c = stub.calls[-1]
    assert c["n_saves"] == T and abs(c["saves_dt"] - 0.01) < 1e-8 and c["dt"] == 0.01 and c["sel"] is None
    with pytest.raises(ValueError):
        ra.rollout_errors(stub, gt, None, None, 0.0, float(saves[-1]), 0.01, saves, [0.123])


# ---- the refusals that need no device --------------------------------------------------------------------------------------------------
def host_engine(**kw):
    pos, cells = synth.grid_mesh(4, 3, 1)
    s, r = synth.cells_to_edges(cells)
    N, E = pos.shape[0], s.size
    e = Engine(9, 3, 2, L=32, mps=1, device=MGN_DEVICE_NONE, **kw)
    return e, s, r, N, E


def test_argument_refusals_host_only(lib_built):
    e, s, r, N, E = host_engine()
    e.set_graph(s, r, N)
    oh, ef = np.zeros((N, 7), np.float32), np.zeros((E, 3), np.float32)
    gt = np.zeros((3, N, 2), np.float32)

    def call(gt=gt, n_saves=3, **kw):
        return e.rollout_eval("Euler", gt[0], oh, ef, gt, 0.0, 0.02, 0.01, n_saves, dt=0.01, **kw)

    cases = [(dict(n_saves=4), _capi.MGN_E_ARG),                                           # n_gt < n_saves
             (dict(sel=np.array([0, 2 * N], np.int32)), _capi.MGN_E_ARG),                  # outside [0, N * O)
             (dict(sel=np.array([-1], np.int32)), _capi.MGN_E_ARG),
             (dict(sel=np.array([0], np.int32), sel_index_base=1), _capi.MGN_E_ARG),
             (dict(sel=np.array([2 * N], np.int32), sel_index_base=2), _capi.MGN_E_ARG),
             (dict(sel=np.array([2 * N], np.int32), sel_index_base=1), _capi.MGN_E_HIP),   # well-formed: a host-only handle has no compute path
             (dict(), _capi.MGN_E_HIP)]
    for kw, code in cases:
        with pytest.raises(MgnError) as ei:
            call(**kw)
        assert ei.value.code == code, (kw, ei.value)
    # NULL descriptors
    lib = _capi.load()
    d = _capi.MgnRolloutDesc()
    assert lib.mgn_rollout_eval(e.h, C.byref(d), None) == _capi.MGN_E_ARG
    assert lib.mgn_rollout_eval(e.h, C.byref(d), C.byref(_capi.MgnRolloutEvalDesc())) == _capi.MGN_E_ARG      # gt NULL
    ev = _capi.MgnRolloutEvalDesc()
    ev.gt, ev.n_gt, ev.n_sel = _capi.f32(gt), 3, -1
    assert lib.mgn_rollout_eval(e.h, C.byref(d), C.byref(ev)) == _capi.MGN_E_ARG
    e.close()


def test_partitioned_handle_is_unsupported_and_says_where_to_go(lib_built):
    e, s, r, N, E = host_engine(rank=0, nranks=2)
    gt = np.zeros((3, N, 2), np.float32)
    ev = _capi.MgnRolloutEvalDesc()
    ev.gt, ev.n_gt = _capi.f32(gt), 3
    d = _capi.MgnRolloutDesc()
    d.n_saves = 3
    assert e.lib.mgn_rollout_eval(e.h, C.byref(d), C.byref(ev)) == _capi.MGN_E_UNSUPPORTED
    msg = e.lib.mgn_last_error(e.h).decode()
    assert "mgn_rollout" in msg.replace("mgn_rollout_eval", "") and "host" in msg
    e.close()
