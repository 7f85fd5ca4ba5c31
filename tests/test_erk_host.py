"""Explicit Runge-Kutta by tableau without a GPU: mgn_erk_named / mgn_erk_check (the flat tableau of include/mgn_hip.h), the named methods
against their rationals, the order conditions and a NumPy integrator on the returned arrays, every refusal of the check, the ABI version
the new symbols leave alone, the calls Engine.rollout / rollout_eval make for a tableau (a recorder in place of the library), the answer
of a host-only handle, reference_api's fixed_step with the new names, and the Julia shim's text."""
import ctypes as C
import inspect
import os
import re
from fractions import Fraction as Fr

import numpy as np
import pytest

import test_julia_shim as js
from mgn_amd import Engine, ErkTableau, GroupEngine, MgnError, _capi, erk_tableau
from mgn_amd import reference_api as ra
from test_rollout_eval_host import StubEngine, canned, host_engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("Euler", "Heun", "Midpoint", "Ralston", "RK4", "BS3", "DP5", "Tsit5")
NEW_SYMBOLS = ("mgn_erk_named", "mgn_erk_check", "mgn_rollout_erk", "mgn_rollout_eval_erk", "mgn_group_rollout_erk",
               "mgn_group_rollout_eval_erk", "mgn_solver_grad_erk")


def F(text):
    return [Fr(x) for x in text.split()]


# name: (order, fsal, rows of A, b, c, btilde or None, betas) -- the methods' coefficients as rationals (Hairer, Norsett, Wanner; Bogacki-Shampine 1989; Dormand-Prince 1980)
RATIONALS = {
    "Euler": (1, False, [[]], F("1"), F("0"), None, (0.0, 0.0)),
    "Heun": (2, False, [[], F("1")], F("1/2 1/2"), F("0 1"), None, (0.0, 0.0)),
    "Midpoint": (2, False, [[], F("1/2")], F("0 1"), F("0 1/2"), None, (0.0, 0.0)),
    "Ralston": (2, False, [[], F("2/3")], F("1/4 3/4"), F("0 2/3"), None, (0.0, 0.0)),
    "RK4": (4, False, [[], F("1/2"), F("0 1/2"), F("0 0 1")], F("1/6 1/3 1/3 1/6"), F("0 1/2 1/2 1"), None, (0.0, 0.0)),
    "BS3": (3, True, [[], F("1/2"), F("0 3/4"), F("2/9 1/3 4/9")], F("2/9 1/3 4/9 0"), F("0 1/2 3/4 1"), F("-5/72 1/12 1/9 -1/8"), (0.0, 0.0)),
    "DP5": (5, True, [[], F("1/5"), F("3/40 9/40"), F("44/45 -56/15 32/9"), F("19372/6561 -25360/2187 64448/6561 -212/729"),
                      F("9017/3168 -355/33 46732/5247 49/176 -5103/18656"), F("35/384 0 500/1113 125/192 -2187/6784 11/84")],
            F("35/384 0 500/1113 125/192 -2187/6784 11/84 0"), F("0 1/5 3/10 4/5 8/9 1 1"),
            F("71/57600 0 -71/16695 71/1920 -17253/339200 22/525 -1/40"), (0.17, 0.04)),
}


def named(name):
    tab = np.full(_capi.MGN_ERK_TABLEAU_DOUBLES, np.nan)
    assert _capi.load().mgn_erk_named(_capi.ERK_NAMES[name], tab.ctypes.data_as(C.POINTER(C.c_double))) == _capi.MGN_OK
    return tab


def check(tab):
    tab = np.ascontiguousarray(tab, np.float64)
    return _capi.load().mgn_erk_check(tab.ctypes.data_as(C.POINTER(C.c_double)))


@pytest.mark.parametrize("name", NAMES)
def test_named_tableau_passes_the_check_and_fills_all_76_doubles(lib_built, name):
    tab = named(name)
    assert np.isfinite(tab).all() and check(tab) == _capi.MGN_OK
    t = erk_tableau(name)
    assert isinstance(t, ErkTableau) and np.array_equal(t.tab, tab) and t.name == name
    s = t.stages
    assert t.A.shape == (s, s) and np.array_equal(t.A, np.tril(t.A, -1)) and t.b.shape == t.c.shape == t.btilde.shape == (s,)
    inside = np.zeros(76, bool)                                   # nothing outside the header, the lower triangle, b, c and btilde
    inside[:6] = True
    for i in range(s):
        inside[6 + 7 * i:6 + 7 * i + i] = True
        inside[[55 + i, 62 + i, 69 + i]] = True
    assert not tab[~inside].any()


@pytest.mark.parametrize("name", sorted(RATIONALS))
def test_named_tableau_is_its_rationals_rounded_once(lib_built, name):
    p, fsal, rows, b, c, bt, betas = RATIONALS[name]
    t = erk_tableau(name)
    assert (t.stages, t.order, t.fsal, t.embedded, t.betas) == (len(b), p, fsal, bt is not None, betas)
    for i, row in enumerate(rows):
        assert t.A[i, :i].tolist() == [float(x) for x in row], i                 # float(Fraction) rounds the rational once
    assert t.b.tolist() == [float(x) for x in b] and t.c.tolist() == [float(x) for x in c]
    assert t.btilde.tolist() == ([float(x) for x in bt] if bt is not None else [0.0] * len(b))


def test_tsit5_tableau_is_the_one_the_library_drives(lib_built):
    t = erk_tableau("Tsit5")
    assert (t.stages, t.order, t.fsal, t.embedded, t.betas) == (7, 5, True, True, (0.0, 0.0))
    assert t.c.tolist() == list(ra.TSIT5_C)
    for i in range(7):
        assert t.A[i, :i].tolist() == list(ra.TSIT5_A[i][:i]), i
    assert t.b[:6].tolist() == list(ra.TSIT5_A[6]) and t.b[6] == 0.0
    w = np.zeros(7)
    assert _capi.load().mgn_tsit5_interp_weights(1.0, w.ctypes.data_as(C.POINTER(C.c_double))) == _capi.MGN_OK
    # b(1) is a Horner sum of four polynomial coefficients of size up to 88.2: a few ulps of that, not of b
    assert np.abs(w - t.b).max() <= 4 * 88.2 * np.finfo(np.float64).eps


def order_residuals(A, b, c, upto):
    """the largest residual of the rooted-tree order conditions of orders 1 .. upto (at most 4)"""
    Ac = A @ c
    conds = [[b.sum() - 1.0], [b @ c - 1 / 2], [b @ c ** 2 - 1 / 3, b @ Ac - 1 / 6],
             [b @ c ** 3 - 1 / 4, (b * c) @ Ac - 1 / 8, b @ (A @ c ** 2) - 1 / 12, b @ (A @ Ac) - 1 / 24]]
    return max(abs(r) for order in conds[:upto] for r in order)


@pytest.mark.parametrize("name", NAMES)
def test_order_conditions(lib_built, name):
    t = erk_tableau(name)
    assert np.abs(t.A.sum(axis=1) - t.c).max() <= 1e-13                         # c_i = sum_j A[i][j], which the conditions below assume
    assert order_residuals(t.A, t.b, t.c, min(t.order, 4)) <= 1e-13
    if t.embedded:
        assert abs(t.btilde.sum()) <= 1e-13
        assert order_residuals(t.A, t.b - t.btilde, t.c, min(t.order - 1, 4)) <= 1e-13


def integrate(t, dt, T):
    """y' = -y + sin t from y(0) = 1 to T with the tableau's arrays, in float64"""
    A, b, c, s = t.A, t.b, t.c, t.stages
    f = lambda tt, y: -y + np.sin(tt)      # noqa: E731
    y, tt = 1.0, 0.0
    for _ in range(int(round(T / dt))):
        k = []
        for i in range(s):
            k.append(f(tt + c[i] * dt, y + dt * sum(A[i, j] * k[j] for j in range(i))))
        y, tt = y + dt * sum(b[i] * k[i] for i in range(s)), tt + dt
    return y


@pytest.mark.parametrize("name", NAMES)
def test_numpy_integrator_shows_the_stated_order(lib_built, name):
    t = erk_tableau(name)
    T = 2.0
    exact = 1.5 * np.exp(-T) + 0.5 * (np.sin(T) - np.cos(T))
    dts = [0.5 / 2 ** k for k in range(5)]                                      # four halvings
    errs = [abs(integrate(t, dt, T) - exact) for dt in dts]
    slope = np.polyfit(np.log(dts), np.log(errs), 1)[0]
    print(name, "errors", ["%.3e" % e for e in errs], "slope %.3f" % slope)
    assert min(errs) > 1e-14                                                    # above round-off: the slope is the method's
    assert slope >= t.order - 0.3


def test_every_refusal_of_the_check(lib_built):
    lib = _capi.load()
    assert lib.mgn_erk_check(None) == _capi.MGN_E_ARG and lib.mgn_erk_named(4, None) == _capi.MGN_E_ARG
    tab = np.zeros(76)
    for bad in (-1, 8, 100):
        assert lib.mgn_erk_named(bad, tab.ctypes.data_as(C.POINTER(C.c_double))) == _capi.MGN_E_ARG, bad
    rk4, bs3 = named("RK4"), named("BS3")
    assert check(rk4) == check(bs3) == _capi.MGN_OK

    def changed(base, **at):
        t = base.copy()
        for k, v in at.items():
            t[int(k[1:])] = v
        return t

    A, B, Cc, BT = 6, 55, 62, 69
    bad = {
        "stages 0": changed(rk4, i0=0), "stages 8": changed(rk4, i0=8), "stages 3.5": changed(rk4, i0=3.5),
        "order 0": changed(rk4, i1=0), "order 2.5": changed(rk4, i1=2.5), "fsal 0.5": changed(rk4, i2=0.5), "fsal 2": changed(rk4, i2=2),
        "embedded 0.5": changed(rk4, i3=0.5), "embedded 2": changed(rk4, i3=2),
        "nan in c": changed(rk4, **{"i%d" % (Cc + 1): np.nan}), "inf outside the block": changed(rk4, i75=np.inf),
        "diagonal": changed(rk4, **{"i%d" % (A + 7 * 1 + 1): 0.5}), "upper": changed(rk4, **{"i%d" % (A + 7 * 1 + 3): 0.5}),
        "sum b": changed(rk4, **{"i%d" % B: 1 / 6 + 1e-9}),
        "embedded, sum btilde": changed(bs3, **{"i%d" % BT: -5 / 72 + 1e-9}),
        "embedded flag on a tableau whose btilde does not sum to 0": changed(rk4, i3=1, **{"i%d" % BT: 0.25}),
        "fsal, b_s": changed(bs3, **{"i%d" % (B + 3): 1e-12}),                  # (sum b stays within 1e-10)
        "fsal, c_s": changed(bs3, **{"i%d" % (Cc + 3): 1 - 1e-12}),
        "fsal, last row": changed(bs3, **{"i%d" % (A + 7 * 3 + 1): np.nextafter(1 / 3, 1)}),
        "fsal on RK4": changed(rk4, i2=1),
        "beta1 < 0": changed(bs3, i4=-0.1), "beta2 < 0": changed(bs3, i5=-0.1),
    }
    for why, t in bad.items():
        assert check(t) == _capi.MGN_E_ARG, why
    # what the check leaves alone: entries outside the s x s block, a sum of b within 1e-10, btilde without the embedded flag
    assert check(changed(named("Heun"), **{"i%d" % (A + 7 * 0 + 5): 3.0})) == _capi.MGN_OK
    assert check(changed(rk4, **{"i%d" % B: 1 / 6 + 1e-12})) == _capi.MGN_OK
    assert check(changed(rk4, **{"i%d" % BT: 0.25})) == _capi.MGN_OK
    with pytest.raises(ValueError):
        ErkTableau(bad["diagonal"])


def test_custom_tableau_from_arrays(lib_built):
    rk4 = erk_tableau("RK4")
    mine = erk_tableau(rk4.A, rk4.b, rk4.c, order=4)
    assert np.array_equal(mine.tab, rk4.tab) and not mine.embedded
    bs3 = erk_tableau("BS3")
    mine = erk_tableau(bs3.A, bs3.b, bs3.c, bs3.btilde, order=3, fsal=True)
    assert np.array_equal(mine.tab, bs3.tab) and mine.embedded and mine.fsal
    assert erk_tableau(bs3.A, bs3.b, bs3.c, bs3.btilde, order=3, fsal=True, betas=(0.2, 0.05)).betas == (0.2, 0.05)
    with pytest.raises(ValueError):
        erk_tableau(np.ones((2, 2)), [0.5, 0.5], [0, 1], order=2)               # not explicit
    with pytest.raises(ValueError):
        erk_tableau(np.zeros((8, 8)), np.full(8, 1 / 8), np.zeros(8), order=1)  # more than seven stages
    with pytest.raises(KeyError):
        erk_tableau("RK45")


def test_abi_version_stays_4_and_every_new_symbol_is_bound(lib_built):
    hdr = open(os.path.join(ROOT, "include", "mgn_hip.h")).read()
    assert re.search(r"^#define MGN_ABI_VERSION 4\s*$", hdr, flags=re.M)
    assert _capi.ABI_VERSION == 4 and _capi.load().mgn_abi_version() == 4
    jl = js._strip_jl_comments(open(os.path.join(js.JULIA_DIR, "MGNHip.jl")).read())
    assert re.search(r"^const ABI_VERSION = 4\b", jl, flags=re.M)
    assert re.search(r"^#define MGN_ERK_MAX_STAGES 7\s*$", hdr, flags=re.M) and re.search(r"^#define MGN_ERK_TABLEAU_DOUBLES 76\s*$", hdr, flags=re.M)
    assert (_capi.MGN_ERK_MAX_STAGES, _capi.MGN_ERK_TABLEAU_DOUBLES) == (7, 76)
    m = re.search(r"typedef enum mgn_erk_name \{([^}]*)\} mgn_erk_name;", hdr)
    assert m
    names = dict((k.strip(), int(v)) for k, v in (item.split("=") for item in m.group(1).split(",")))
    assert names == {"MGN_ERK_" + k.upper(): v for k, v in _capi.ERK_NAMES.items()}
    protos = js.c_prototypes()
    for sym in NEW_SYMBOLS:
        assert sym in protos and sym in _capi.PROTOTYPES and hasattr(_capi.load(), sym), sym
        assert len(_capi.PROTOTYPES[sym][1]) == len(protos[sym][1]), sym
    # no struct moved
    assert [n for n, _ in _capi.MgnRolloutDesc._fields_] == [n for n, _ in js.c_struct("mgn_rollout_desc")]


class RecorderLib:
    """The library with the four rollout symbols replaced by recorders of what they are handed."""

    FIELDS = ("solver", "t0", "t1", "dt", "saves_dt", "n_saves", "abstol", "reltol", "inflow_rule", "time_f64", "dt_f64", "n_frames")

    def __init__(self, real):
        self._real, self.calls = real, []

    def _record(self, name, d, tab=None, adaptive=None):
        rec = dict({f: getattr(d._obj, f) for f in self.FIELDS}, call=name)
        if tab is not None:
            rec.update(tab=np.ctypeslib.as_array(tab, shape=(76,)).copy(), adaptive=adaptive)
        self.calls.append(rec)
        return _capi.MGN_OK

    def mgn_rollout(self, h, d):
        return self._record("mgn_rollout", d)

    def mgn_rollout_eval(self, h, d, e):
        return self._record("mgn_rollout_eval", d)

    def mgn_rollout_erk(self, h, d, tab, adaptive):
        return self._record("mgn_rollout_erk", d, tab, adaptive)

    def mgn_rollout_eval_erk(self, h, d, e, tab, adaptive):
        return self._record("mgn_rollout_eval_erk", d, tab, adaptive)

    def __getattr__(self, name):
        return getattr(self._real, name)


def test_engine_routes_tableaux_to_the_erk_symbols_and_keeps_todays_calls(lib_built):
    e, s, r, N, E = host_engine()
    e.set_graph(s, r, N)
    rec = e.lib = RecorderLib(e.lib)
    oh, ef = np.zeros((N, 7), np.float32), np.zeros((E, 3), np.float32)
    gt = np.zeros((3, N, 2), np.float32)
    a = (gt[0], oh, ef)
    grid = (0.0, 0.02, 0.01, 3)

    def last():
        return rec.calls[-1]

    # RK4 has no embedded pair: fixed steps whatever `adaptive` says
    for kw in (dict(), dict(adaptive=True), dict(adaptive=False)):
        e.rollout("RK4", *a, *grid, dt=0.005, **kw)
        assert last()["call"] == "mgn_rollout_erk" and last()["adaptive"] == 0 and abs(last()["dt"] - 0.005) < 1e-9
        assert np.array_equal(last()["tab"], named("RK4"))
        e.rollout_eval("RK4", *a, gt, *grid, dt=0.005, **kw)
        assert last()["call"] == "mgn_rollout_eval_erk" and last()["adaptive"] == 0 and np.array_equal(last()["tab"], named("RK4"))
    # BS3 and DP5 follow the keyword, as "Tsit5" does
    for name in ("BS3", "DP5"):
        e.rollout(name, *a, *grid)
        assert last()["call"] == "mgn_rollout_erk" and last()["adaptive"] == 1 and last()["dt"] == 0.0
        e.rollout(name, *a, *grid, dt=0.005, adaptive=False)
        assert last()["adaptive"] == 0 and np.array_equal(last()["tab"], named(name))
        e.rollout_eval(name, *a, gt, *grid, time_type=np.float64)
        assert last()["call"] == "mgn_rollout_eval_erk" and last()["adaptive"] == 1 and last()["time_f64"] == 1
        e.rollout_eval(name, *a, gt, *grid, dt=0.005, adaptive=False)
        assert last()["adaptive"] == 0
    # an ErkTableau object, embedded or not
    e.rollout(erk_tableau("Heun"), *a, *grid, dt=0.01)
    assert last()["call"] == "mgn_rollout_erk" and last()["adaptive"] == 0 and np.array_equal(last()["tab"], named("Heun"))
    e.rollout(erk_tableau("Tsit5"), *a, *grid)
    assert last()["call"] == "mgn_rollout_erk" and last()["adaptive"] == 1 and np.array_equal(last()["tab"], named("Tsit5"))
    # "Euler" and "Tsit5" build exactly today's descriptors and calls
    e.rollout("Euler", *a, *grid, dt=0.01)
    assert last()["call"] == "mgn_rollout" and last()["solver"] == 0 and "tab" not in last()
    e.rollout("Tsit5", *a, *grid)
    assert last()["call"] == "mgn_rollout" and last()["solver"] == 1 and "tab" not in last()
    e.rollout("Tsit5", *a, *grid, dt=0.004, adaptive=False)
    assert last()["call"] == "mgn_rollout" and last()["solver"] == 2
    e.rollout_eval("Euler", *a, gt, *grid, dt=0.01)
    assert last()["call"] == "mgn_rollout_eval" and last()["solver"] == 0
    e.rollout_eval("Tsit5", *a, gt, *grid)
    assert last()["call"] == "mgn_rollout_eval" and last()["solver"] == 1
    with pytest.raises(KeyError):
        e.rollout("RK45", *a, *grid)
    with pytest.raises(TypeError):
        e.rollout(4, *a, *grid)
    e.lib = rec._real
    e.close()
    for cls in (Engine, GroupEngine):
        for name in ("rollout", "rollout_eval"):
            assert inspect.signature(getattr(cls, name)).parameters["adaptive"].default is True, (cls, name)


def test_host_only_handle_answers_the_erk_calls(lib_built):
    e, s, r, N, E = host_engine()
    e.set_graph(s, r, N)
    oh, ef = np.zeros((N, 7), np.float32), np.zeros((E, 3), np.float32)
    gt = np.zeros((3, N, 2), np.float32)
    for name in ("RK4", "BS3"):
        with pytest.raises(MgnError) as ei:
            e.rollout(name, gt[0], oh, ef, 0.0, 0.02, 0.01, 3, dt=0.005, adaptive=False)
        assert ei.value.code == _capi.MGN_E_HIP
        with pytest.raises(MgnError) as ei:
            e.rollout_eval(name, gt[0], oh, ef, gt, 0.0, 0.02, 0.01, 3, dt=0.005, adaptive=False)
        assert ei.value.code == _capi.MGN_E_HIP
    # a bad tableau is refused before anything else, on this handle too
    d, keep = e._rollout_desc("Euler", gt[0], oh, ef, 0.0, 0.02, 0.01, 3, 0.005, None, None, None, 1e-6, 1e-3, "reference", np.float32)
    out = np.zeros((3, N, 2), np.float32)
    d.out = _capi.f32(out)
    bad = named("RK4")
    bad[0] = 9
    ev = _capi.MgnRolloutEvalDesc()
    ev.gt, ev.n_gt = _capi.f32(gt), 3
    p = bad.ctypes.data_as(C.POINTER(C.c_double))
    assert e.lib.mgn_rollout_erk(e.h, C.byref(d), p, 0) == _capi.MGN_E_ARG
    assert "mgn_erk_check" in e.lib.mgn_last_error(e.h).decode()
    assert e.lib.mgn_rollout_eval_erk(e.h, C.byref(d), C.byref(ev), p, 0) == _capi.MGN_E_ARG
    assert e.lib.mgn_rollout_erk(e.h, C.byref(d), None, 0) == _capi.MGN_E_ARG
    assert e.lib.mgn_rollout_eval_erk(e.h, C.byref(d), C.byref(ev), None, 0) == _capi.MGN_E_ARG
    good = named("RK4").ctypes.data_as(C.POINTER(C.c_double))
    assert e.lib.mgn_rollout_erk(e.h, C.byref(d), good, 0) == _capi.MGN_E_HIP
    # the training entry point: the tableau, then the step mode, then the handle
    g, lv, o = np.zeros(e.param_count, np.float32), C.c_float(), _capi.MgnSolverGradOpts()

    def train(tab_ptr):
        return e.lib.mgn_solver_grad_erk(e.h, C.byref(d), tab_ptr, C.byref(o), _capi.f32(gt), None, None, 0.0, _capi.f32(g), g.size, C.byref(lv))

    assert train(p) == _capi.MGN_E_ARG and train(None) == _capi.MGN_E_ARG
    o.adaptive = 1
    assert train(good) == _capi.MGN_E_UNSUPPORTED
    o.adaptive = 0
    assert train(good) == _capi.MGN_E_HIP
    with pytest.raises(MgnError) as ei:
        e.solver_grad_erk("RK4", gt[0], oh, ef, gt, 0.0, 0.02, 0.01, 3, 0.005)
    assert ei.value.code == _capi.MGN_E_HIP
    del keep
    e.close()


def test_reference_api_takes_the_new_names_and_treats_fixed_step_as_for_tsit5():
    gt, pred = canned()
    N = gt.shape[1]
    mask = np.array([1, 2, 4, 8, 11], np.int32)
    stub = StubEngine(pred)
    interval = (0.0, 0.01, 0.04)

    def vs(**kw):
        ra.validation_step(stub, gt, None, None, interval, mask, inflow_mask=np.ones(N), **kw)
        return stub.calls[-1]

    for name in ("RK4", "BS3", "DP5", "Heun"):
        c = vs(solver=name, solver_dt=0.01, fixed_step=True)
        assert c["adaptive"] is False and c["dt"] == 0.01 and c["solver"] == name
        for kw in (dict(solver=name, solver_dt=0.01), dict(solver=name), dict(solver=name, fixed_step=True)):
            assert "adaptive" not in vs(**kw), kw
    saves = np.arange(gt.shape[0], dtype=np.float32) * np.float32(0.01)
    ra.rollout_errors(stub, gt, None, None, 0.0, float(saves[-1]), 0.01, saves, [saves[2]], solver="BS3", fixed_step=True)
    assert stub.calls[-1]["adaptive"] is False and stub.calls[-1]["solver"] == "BS3"
    ra.rollout_errors(stub, gt, None, None, 0.0, float(saves[-1]), None, saves, [saves[2]], solver="BS3", fixed_step=True)
    assert "adaptive" not in stub.calls[-1]
    # Euler and Tsit5 as before
    assert "adaptive" not in vs(solver="Euler", solver_dt=0.01, fixed_step=True)
    assert vs(solver="Tsit5", solver_dt=0.01, fixed_step=True)["adaptive"] is False


def test_julia_shim_names_the_tableaux_and_calls_the_erk_symbols():
    text = js._strip_jl_comments(open(os.path.join(js.JULIA_DIR, "MGNHip.jl")).read())
    m = re.search(r"const ERK_NAMES = \(([^)]*)\)", text)
    assert m
    names = dict((k.strip(), int(v)) for k, v in (item.split("=") for item in m.group(1).split(",")))
    assert names == _capi.ERK_NAMES
    calls = {sym: types for sym, _, types, _ in js.julia_ccalls(os.path.join(js.JULIA_DIR, "MGNHip.jl"))}
    assert calls["mgn_erk_named"] == ["Int32", "Ptr{Float64}"] and calls["mgn_erk_check"] == ["Ptr{Float64}"]
    assert calls["mgn_rollout_erk"] == ["Ptr{Cvoid}", "Ref{MgnRolloutDesc}", "Ptr{Float64}", "Int32"]
    m = re.search(r"@ccall\s+LIB\.mgn_rollout_eval_erk\((.*?)\)::Cint", text, flags=re.S)
    assert m
    types = [a.rsplit("::", 1)[1].strip() for a in js._split_top(m.group(1))]
    assert types == ["Ptr{Cvoid}", "Ref{MgnRolloutDesc}", "Ref{MgnRolloutEvalDesc}", "Ptr{Float64}", "Int32"]
    assert len(types) == len(js.c_prototypes()["mgn_rollout_eval_erk"][1])
    m = re.search(r"@ccall\s+LIB\.mgn_solver_grad_erk\((.*?)\)::Cint", text, flags=re.S)
    assert m
    types = [re.sub(r"^.*::", "", a).strip() for a in js._split_top(m.group(1))]
    assert types == ["Ptr{Cvoid}", "Ref{MgnRolloutDesc}", "Ptr{Float64}", "Ref{MgnSolverGradOpts}", "Ptr{Float32}", "Ptr{Float32}", "Ptr{Float32}",
                     "Float32", "Ptr{Float32}", "Csize_t", "Ref{Float32}"]
    assert len(types) == len(js.c_prototypes()["mgn_solver_grad_erk"][1])
    assert re.search(r"^function solver_grad_erk\(", text, flags=re.M) and re.search(r"^\s+native_rollout,[^\n]*\bsolver_grad_erk\b", text, flags=re.M)      # (a line of the export list)
    assert "native_solver_train_step drives Euler() and Tsit5(); got" not in text
    assert "native_rollout drives Euler and Tsit5; got" not in text
    assert re.search(r"nameof\(typeof\(solver\)\)", text)
    # the two three-way descriptor lines stay
    assert len(re.findall(r"MgnRolloutDesc\(name == :Euler \? 0 : \(fixed_step \? 2 : 1\),", text)) == 2
