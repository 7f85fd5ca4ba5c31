"""Device-resident parameters and the device Adam (mgn_set_params_dev, mgn_get_params_dev, mgn_adam_init / _update / _state) without
a GPU: the symbols are declared, exported and bound on the ctypes and the Julia side, a host-only handle refuses all five with
MGN_E_HIP, the argument refusals come first (they need no device), and the float32 restatement the GPU tests compare bits with
(tests/adam_f32.py) agrees with checkpoint.Adam, the tested twin of Optimisers.Adam."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import adam_f32
import test_julia_shim as js
from mgn_amd import MGN_DEVICE_NONE, Engine, _capi
from mgn_amd.checkpoint import Adam

HEADER = os.path.join(os.path.dirname(js.JULIA_DIR), "include", "mgn_hip.h")
F = np.float32
f32p, f64p = C.POINTER(C.c_float), C.POINTER(C.c_double)
WANT = {
    "mgn_set_params_dev": [("mgn_handle", 1), ("f32", 1), ("size", 0)],
    "mgn_get_params_dev": [("mgn_handle", 1), ("f32", 1), ("size", 0)],
    "mgn_adam_init": [("mgn_handle", 1), ("mgn_adam_desc", 1)],
    "mgn_adam_update": [("mgn_handle", 1), ("f32", 1), ("size", 0)],
    "mgn_adam_state": [("mgn_handle", 1), ("i32", 0), ("f32", 1), ("f32", 1), ("f64", 1)],
}


def test_declared_exported_and_bound(lib_built):
    lib = _capi.load()
    protos = js.c_prototypes()
    for sym, want in WANT.items():
        assert hasattr(lib, sym), sym
        assert protos[sym] == (("i32", 0), want), sym
        restype, argtypes = _capi.PROTOTYPES[sym]
        assert restype is C.c_int and len(argtypes) == len(want), sym
    assert js.c_struct("mgn_adam_desc") == [(n, ("f32", 0)) for n in ("eta", "beta1", "beta2", "epsilon")]
    assert [(n, t) for n, t in _capi.MgnAdamDesc._fields_] == [(n, C.c_float) for n in ("eta", "beta1", "beta2", "epsilon")]
    lib.mgn_abi_version.restype = C.c_int
    assert lib.mgn_abi_version() == 4                       # only additions: the version stands
    assert re.search(r"#define\s+MGN_ABI_VERSION\s+4\b", open(HEADER).read())


def test_python_surface():
    import mgn_amd
    for name in ("set_params_dev", "get_params", "adam_init", "adam_update", "adam_state", "set_adam_state"):
        assert callable(getattr(Engine, name)), name
    for name in ("set_params_dev", "adam_init", "adam_update", "adam_state", "set_adam_state"):     # group wrappers are not part of this
        assert not hasattr(mgn_amd.GroupEngine, name), name
    assert not any(n.startswith("mgn_group") and ("adam" in n or n.endswith("params_dev")) for n in _capi.PROTOTYPES)


def test_julia_binding():
    path = os.path.join(js.JULIA_DIR, "MGNHip.jl")
    text = js._strip_jl_comments(open(path).read())
    calls = {}
    for sym, ret, types, args in js.julia_ccalls(path):
        calls.setdefault(sym, []).append((ret, types, args))
    for sym, want in WANT.items():
        if sym == "mgn_adam_init":
            continue
        assert calls.get(sym), sym
        for ret, types, args in calls[sym]:
            assert js._compatible(js._JL[ret], ("i32", 0)) and len(types) == len(want) == len(args), sym
            for k, (t, c) in enumerate(zip(types, want)):
                assert js._compatible(js._JL[t], c), (sym, k, t, c)
    # mgn_adam_init takes a struct by reference: an @ccall, whose argument types stand behind the values
    m = re.search(r"@ccall\s+LIB\.mgn_adam_init\((.*?)\)::Cint", text, re.S)
    assert m and [a.split("::")[1].strip() for a in js._split_top(m.group(1))] == ["Ptr{Cvoid}", "Ref{MgnAdamDesc}"]
    assert js.julia_struct(path, "MgnAdamDesc") == [(n, "Float32") for n in ("eta", "beta1", "beta2", "epsilon")]
    for fn in ("adam_init!", "adam_update!"):
        assert re.search(r"^export\b[^\n]*" + re.escape(fn), text, re.M), fn
        assert re.search(r"^function " + re.escape(fn) + r"\(", text, re.M), fn
    assert re.search(r"^const ABI_VERSION = 4\b", text, re.M)


@pytest.fixture()
def host_engine(lib_built):
    e = Engine(9, 3, 2, L=32, hidden_layers=2, mps=1, device=MGN_DEVICE_NONE)
    yield e
    e.close()


def _calls(e, n, ps, bt, desc):
    """the five calls with valid arguments"""
    lib, h = e.lib, e.h
    return {
        "mgn_set_params_dev": lambda: lib.mgn_set_params_dev(h, _capi.f32(ps), n),
        "mgn_get_params_dev": lambda: lib.mgn_get_params_dev(h, _capi.f32(ps), n),
        "mgn_adam_init": lambda: lib.mgn_adam_init(h, C.byref(desc)),
        "mgn_adam_update": lambda: lib.mgn_adam_update(h, _capi.f32(ps), n),
        "mgn_adam_state": lambda: lib.mgn_adam_state(h, 0, _capi.f32(ps), _capi.f32(ps), bt.ctypes.data_as(f64p)),
    }


def test_host_only_handle_refuses_with_e_hip(host_engine):
    e = host_engine
    n = e.param_count
    ps, bt = np.zeros(n, F), np.zeros(2, np.float64)
    desc = _capi.MgnAdamDesc(1e-3, 0.9, 0.999, 1e-8)
    for name, call in _calls(e, n, ps, bt, desc).items():
        assert call() == _capi.MGN_E_HIP, name
        assert b"host-only" in e.lib.mgn_last_error(e.h), name
    assert e.param_count == n                                # the handle is still there


def test_argument_refusals_need_no_device(host_engine):
    e = host_engine
    lib, h, n = e.lib, e.h, e.param_count
    ps, bt = np.zeros(n + 1, F), np.array([0.9, 0.999], np.float64)
    btp, p = bt.ctypes.data_as(f64p), _capi.f32(ps)
    ARG = _capi.MGN_E_ARG
    # NULL pointers
    assert lib.mgn_set_params_dev(h, None, n) == ARG
    assert lib.mgn_get_params_dev(h, None, n) == ARG
    assert lib.mgn_adam_init(h, None) == ARG
    assert lib.mgn_adam_update(h, None, n) == ARG
    assert lib.mgn_adam_state(h, 0, None, p, btp) == ARG
    assert lib.mgn_adam_state(h, 0, p, None, btp) == ARG
    assert lib.mgn_adam_state(h, 0, p, p, None) == ARG
    for fn in (lib.mgn_set_params_dev, lib.mgn_get_params_dev, lib.mgn_adam_update):
        assert fn(None, p, n) == ARG                         # no handle
    # a wrong length
    for bad in (n - 1, n + 1, 0):
        assert lib.mgn_set_params_dev(h, p, bad) == ARG
        assert lib.mgn_get_params_dev(h, p, bad) == ARG
        assert lib.mgn_adam_update(h, p, bad) == ARG
    # write other than 0 / 1
    for w in (-1, 2):
        assert lib.mgn_adam_state(h, w, p, p, btp) == ARG
    # descriptors: not finite, or outside eta > 0, 0 <= beta < 1, epsilon > 0
    nan, inf = float("nan"), float("inf")
    for bad in ((0.0, 0.9, 0.999, 1e-8), (-1e-3, 0.9, 0.999, 1e-8), (nan, 0.9, 0.999, 1e-8), (inf, 0.9, 0.999, 1e-8),
                (1e-3, 1.0, 0.999, 1e-8), (1e-3, -0.1, 0.999, 1e-8), (1e-3, nan, 0.999, 1e-8),
                (1e-3, 0.9, 1.0, 1e-8), (1e-3, 0.9, -0.5, 1e-8), (1e-3, 0.9, inf, 1e-8),
                (1e-3, 0.9, 0.999, 0.0), (1e-3, 0.9, 0.999, -1e-8), (1e-3, 0.9, 0.999, nan)):
        assert lib.mgn_adam_init(h, C.byref(_capi.MgnAdamDesc(*bad))) == ARG, bad
    # beta = 0 is inside the range: the refusal that remains is the host-only handle's
    assert lib.mgn_adam_init(h, C.byref(_capi.MgnAdamDesc(1e-3, 0.0, 0.0, 1e-8))) == _capi.MGN_E_HIP


def ulp(x):
    return np.spacing(np.abs(np.asarray(x, F)))


@pytest.mark.parametrize("hyper", [dict(eta=1e-3, beta=(0.9, 0.999), epsilon=1e-8), dict(eta=3e-4, beta=(0.8, 0.99), epsilon=1e-6)],
                         ids=["defaults", "other"])
def test_restatement_agrees_with_the_twin(hyper):
    """Three updates of tests/adam_f32.py (every operation one fp32 rounding: what the kernel computes) beside three of
    checkpoint.Adam.update, each from its own setup, on the gradients the GPU test uses (magnitudes 1e-3 .. 1e3, exact zeros mixed in).
    Per element and update |p - p_twin| <= 2e-6 |dx| + 1 ulp(p): the twin forms m / (1 - beta_t) / (sqrt(v / (1 - beta_t)) + eps) * eta
    in float64 and rounds once, the restatement rounds seven times (2^-24 each, about 4e-7 of dx); the rest of the allowance covers
    what 1 - beta is in float32 against float64.  Each optimiser is set up by its own `setup`: the twin's beta_t starts at the double
    (0.9, 0.999), the engine's at the float descriptor's values widened, which keeps 1 - beta_t and the float 1 - beta in step as
    Optimisers does for a Float32 model.  Measured here (NumPy 2.2, x86-64): the largest (|p - p_twin| - ulp(p)) / |dx| is 2.4e-7
    with the defaults and 2.0e-7 with the other set."""
    n = 20011
    rng = np.random.default_rng(11)
    ps0 = (rng.standard_normal(n) * 0.3).astype(F)
    twin = Adam(**hyper)
    st_t, st_r = twin.setup(ps0), adam_f32.setup(n, hyper["beta"])
    p = ps0
    for k in range(3):                                       # every update starts from common parameters; the moments stay each one's own
        g = adam_f32.synthetic_grads(n, 100 + k)
        st_t, p_t = twin.update(st_t, p, g)
        st_r, p_r = adam_f32.update(st_r, p, g, **hyper)
        assert p_r.dtype == st_r["mt"].dtype == st_r["vt"].dtype == F and st_r["beta_t"].dtype == np.float64
        dx = np.abs(p.astype(np.float64) - p_t.astype(np.float64))
        diff = np.abs(p_r.astype(np.float64) - p_t.astype(np.float64))
        print("update %d: max (|p - p_twin| - ulp(p)) / |dx| = %.3g" % (k, float(((diff - ulp(p_t)) / np.maximum(dx, 1e-30)).max())))
        bound = 2e-6 * dx + ulp(p_t)
        assert (diff <= bound).all(), (k, float((diff - bound).max()))
        p = p_t
