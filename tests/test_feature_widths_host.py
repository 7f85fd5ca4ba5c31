"""The width rule without a GPU (include/mgn_hip.h, mgn_config "Widths"): a training entry point on a configuration with a width above L
answers MGN_E_UNSUPPORTED before it looks for a device -- so a host-only handle (MGN_DEVICE_NONE) answers it too, with the width and L
in the text -- while a supported configuration keeps the order of its checks (MGN_E_HIP on such a handle); ln_dims = MGN_LN_ALL, whose
inference runs on the training kernels as well, is refused at creation; the parameter count follows the oracle's layout at every
width.  The device side is tests/test_gpu_feature_widths.py.

The packing description of the training weights (pack_describe, mgn_train.cpp) describes an encoder's first layer as ONE block of at
most L rows.  It is reached from train_prepare and from the MGN_LN_ALL drivers only, both behind the refusals tested here; it also
turns a wide configuration away itself, before it describes a job."""
import numpy as np
import pytest

import mgn_oracle as orc
import width_cases as wc
from mgn_amd import MGN_DEVICE_NONE, Engine, GroupEngine, MgnError, _capi

F32 = np.float32
NARROW = [(32, 32, 32, 32), (9, 3, 2, 32)]


def engine(w, **kw):
    Fn, Fe, O, L = w
    e = Engine(Fn, Fe, O, L, 2, wc.MPS, device=MGN_DEVICE_NONE, **kw)
    s, r, N = wc.mesh()
    e.set_graph(s, r, N)
    return e


def training_calls(e, w):
    """every training entry point of Engine with well-formed arguments: [(name, call)]"""
    Fn, Fe, O, L = w
    s, r, N = wc.mesh()
    E = s.size
    z = lambda *shape: np.zeros(shape, F32)      # noqa: E731
    nf, ef, x, tq = z(N, Fn), z(E, Fe), z(N, O), z(N, O)
    oh = z(N, Fn - O) if Fn > O else None
    mask = np.arange(5, dtype=np.int32)
    gt = z(3, N, O)
    grid = (0.0, 0.02, 0.01, 0.01, 3)            # t0, t1, dt, saves_dt, n_saves
    return [
        ("step", lambda: e.step(nf, ef, tq, mask)),
        ("step_datapoint", lambda: e.step_datapoint(0, mask)),
        ("step_datapoints B=1", lambda: e.step_datapoints([0], mask)),
        ("step_datapoints B=2", lambda: e.step_datapoints([0, 1], mask)),
        ("ode_vjp", lambda: e.ode_vjp(x, oh, ef, x)),
        ("forward_vjp", lambda: e.forward_vjp(nf, ef, tq)),
        ("solver_grad", lambda: e.solver_grad(x, oh, ef, gt, *grid)),
        ("solver_grad_tsit5 fixed", lambda: e.solver_grad_tsit5(x, oh, ef, gt, 0.0, 0.02, 0.01, 3, dt=0.01, adaptive=False)),
        ("solver_grad_tsit5 adaptive", lambda: e.solver_grad_tsit5(x, oh, ef, gt, 0.0, 0.02, 0.01, 3)),
        ("solver_grad_erk", lambda: e.solver_grad_erk("RK4", x, oh, ef, gt, 0.0, 0.02, 0.01, 3, 0.01)),
        ("shooting_grad", lambda: e.shooting_grad(oh, ef, gt, [(0, 1), (1, 2)], [0.0, 0.01], [0.01, 0.02], 0.01, 0.01)),
        # the calls around the resident trajectory compute on the same padded rows
        ("set_trajectory", lambda: e.set_trajectory(gt, dt=0.01, node_type_onehot=oh, ef_raw=ef)),
        ("datapoint_export", lambda: e.datapoint_export(0)),
        ("set_noise", lambda: e.set_noise(np.ones(O, F32), np.ones(N, np.uint8), 1)),
        ("online_norms", lambda: e.online_norms()),
        ("norm_state", lambda: e.norm_state(0)),
        ("set_norm_state", lambda: e.set_norm_state(1, np.zeros(Fe), np.zeros(Fe), 0, 0)),
    ]


@pytest.mark.parametrize("w", wc.WIDE, ids=wc.wide_id)
def test_wide_configurations_are_refused_before_the_device_check(lib_built, w):
    e = engine(w)
    s, r, N = wc.mesh()
    name, width = next((n, v) for n, v in zip(("Fn", "Fe", "O"), w[:3]) if v > w[3])
    for what, call in training_calls(e, w):
        with pytest.raises(MgnError) as ei:
            call()
        assert ei.value.code == _capi.MGN_E_UNSUPPORTED, (what, ei.value)
        text = e.lib.mgn_last_error(e.h).decode()
        assert text in str(ei.value)
        assert f"{name} = {width}" in text and f"L = {w[3]}" in text, (what, text)
        e.set_graph(s, r, N)                        # the handle stays usable
        assert e.N == N
    e.close()


@pytest.mark.parametrize("w", NARROW, ids=lambda w: "Fn%d-Fe%d-O%d-L%d" % w)
def test_supported_widths_keep_the_order_of_their_checks(lib_built, w):
    e = engine(w)
    for what, call in training_calls(e, w):
        with pytest.raises(MgnError) as ei:
            call()
        assert ei.value.code == _capi.MGN_E_HIP, (what, ei.value)
    e.close()


@pytest.mark.parametrize("w,kw,text", [((9, 40, 2, 32), {}, "Fe = 40"), ((9, 3, 2, 32), dict(Fe2=33), "Fe2 = 33"),
                                       ((40, 3, 33, 32), {}, "Fn = 40"), ((32, 3, 33, 32), {}, "O = 33"), ((9, 3, 129, 128), {}, "O = 129")])
def test_the_refusal_names_the_first_width_above_L(lib_built, w, kw, text):
    e = engine(w, **kw)
    Fn, Fe, O, L = w
    s, r, N = wc.mesh()
    with pytest.raises(MgnError) as ei:
        e.step(np.zeros((N, Fn), F32), np.zeros((s.size, Fe), F32), np.zeros((N, O), F32), np.arange(3, dtype=np.int32))
    assert ei.value.code == _capi.MGN_E_UNSUPPORTED
    assert text in str(ei.value) and f"L = {L}" in str(ei.value), str(ei.value)
    e.close()


def test_a_second_edge_set_of_width_L_is_in_range(lib_built):
    e = engine((9, 3, 2, 32), Fe2=32)
    s, r, N = wc.mesh()
    with pytest.raises(MgnError) as ei:
        e.step(np.zeros((N, 9), F32), np.zeros((s.size, 3), F32), np.zeros((N, 2), F32), np.arange(3, dtype=np.int32))
    assert ei.value.code == _capi.MGN_E_HIP
    e.close()


def test_whole_array_layernorm_is_refused_at_creation(lib_built):
    for w in wc.WIDE + [(9, 33, 2, 32), (9, 3, 65, 64)]:
        with pytest.raises(MgnError) as ei:
            Engine(w[0], w[1], w[2], w[3], 2, wc.MPS, device=MGN_DEVICE_NONE, ln_dims=1)
        assert ei.value.code == _capi.MGN_E_ARG, (w, ei.value)
        assert f"L = {w[3]}" in str(ei.value) and "MGN_LN_ALL" in str(ei.value), str(ei.value)
    for L in (32, 64, 128):                         # every width equal to L: created
        Engine(L, L, L, L, 2, wc.MPS, device=MGN_DEVICE_NONE, ln_dims=1).close()
    Engine(33, 64, 33, 32, 2, wc.MPS, device=MGN_DEVICE_NONE, ln_dims=0).close()      # row-wise LayerNorm: inference serves it


@pytest.mark.parametrize("w", wc.WIDE[:1] + NARROW[1:], ids=["wide", "narrow"])
def test_host_only_group(lib_built, w):
    Fn, Fe, O, L = w
    s, r, N = wc.mesh()
    want = _capi.MGN_E_UNSUPPORTED if Fn > L else _capi.MGN_E_HIP
    with GroupEngine(Fn, Fe, O, L, 2, wc.MPS, devices=[MGN_DEVICE_NONE] * 2) as g:
        g.set_graph(s, r, N)
        for _ in range(2):
            with pytest.raises(MgnError) as ei:
                g.step(np.zeros((N, Fn), F32), np.zeros((s.size, Fe), F32), np.zeros((N, O), F32), np.arange(5, dtype=np.int32))
            assert ei.value.code == want and "rank" in str(ei.value), str(ei.value)
            if Fn > L:
                assert f"Fn = {Fn}" in str(ei.value) and f"L = {L}" in str(ei.value)
            g.set_graph(s, r, N)                    # the group stays usable: the partition is rebuilt, the ranks answer
            assert sum(g.rank_engine(k).n_own for k in range(2)) == N


@pytest.mark.parametrize("case", wc.ALL_FORWARD, ids=wc.case_id)
def test_param_count_follows_the_oracles_layout(lib_built, case):
    cfg = wc.cfg_of(case)
    e = Engine(cfg["Fn"], cfg["Fe"], cfg["O"], cfg["L"], cfg["hidden_layers"], cfg["mps"], device=MGN_DEVICE_NONE)
    assert e.param_count == wc.params(cfg).size == orc.param_count(cfg["Fn"], cfg["Fe"], cfg["O"], cfg["L"], cfg["hidden_layers"], cfg["mps"])
    e.close()


def test_the_case_table():
    for name, (Fn, Fe, O, L, hl) in wc.IN_RANGE.items():
        assert max(Fn, Fe, O) <= L and Fn >= O, name
    for w in wc.WIDE:
        assert max(w[:3]) > w[3] and w[0] >= w[2], w
    s, r, N = wc.mesh()
    assert (N, s.size) == (63, 316)
