"""Parameters that stay on the device (mgn_set_params_dev / mgn_get_params_dev) and Optimisers.Adam there (mgn_adam_init / _update /
_state): the loop of the reference (src/MeshGraphNets.jl:364-378) as two calls per iteration with nothing of parameter size crossing
PCIe.  Everything here is compared bit for bit: the two doors for parameters against each other, the Adam kernel against the
float32 restatement of tests/adam_f32.py, the device loop against the host loop, every reader of the parameters after a device-side
update against a fresh engine given the same values through mgn_set_params.

Shapes: the 70-node / 200-edge "small" graph of tests/handle_reuse_inputs.py (three node tiles, seven edge tiles, a hub receiver) and
the 150-point cylinder mesh, mps = 2, T = 3 frames."""
import numpy as np
import pytest
import torch

import adam_f32
import mgn_amd
import mgn_oracle as orc
from mgn_amd import _capi, synth
from mgn_amd import checkpoint as ck
from mgn_amd import engine as eng_mod
from mgn_amd import reference_api as ra

pytestmark = pytest.mark.gpu

F = np.float32
MPS, NTYPES, FE, T = 2, 3, 3, 3
DT = F(0.01)


def small_graph(N=70, E=200):
    """handle_reuse_inputs.small_graph: a hub receiver, node 0 sending and receiving, the last N // 8 nodes without an incoming edge"""
    s, r = synth.random_graph(N, E, 7)
    r[:E // 4] = 3
    s[E // 2: E // 2 + E // 8] = 0
    r[E - E // 8:] = 0
    return s, r


class Problem:
    """graph, a trajectory of T frames, the inputs of a plain step(), a mask that lists no node twice"""

    def __init__(self, O, kind="small", Fe2=None):
        if kind == "small":
            self.s, self.r = small_graph()
            self.N = 70
        else:
            pos, cells, _, _ = synth.mesh_cyl(1234, 150)
            self.s, self.r = synth.cells_to_edges(cells)
            self.N = pos.shape[0]
        N, E = self.N, self.s.size
        self.O, self.Fn, self.Fe2 = O, O + NTYPES, Fe2
        rng = np.random.default_rng(N + 31 * O)
        base = rng.standard_normal((N, O))
        self.frames = (base[None] + 0.01 * rng.standard_normal((T, N, O))).astype(F)
        self.onehot = ra.one_hot(rng.integers(0, NTYPES, N), NTYPES).astype(F)
        self.ef_raw = rng.standard_normal((E, FE)).astype(F)
        self.nf = rng.standard_normal((N, self.Fn)).astype(F)
        self.ef = rng.standard_normal((E, FE)).astype(F)
        self.target = rng.standard_normal((N, O)).astype(F)
        self.mask = np.sort(rng.choice(N, int(0.6 * N), replace=False)).astype(np.int32)
        if Fe2:
            self.s2, self.r2 = synth.random_graph(N, 40, 9)
            self.ef2 = rng.standard_normal((40, Fe2)).astype(F)

    def params(self, L, hl, seed=7):
        return orc.init_params(self.Fn, FE, self.O, L, hl, MPS, seed, 0.1, Fe2=self.Fe2).astype(F)

    def engine(self, L, hl, **kw):
        e = mgn_amd.Engine(self.Fn, FE, self.O, L, hl, MPS, Fe2=self.Fe2, **kw)
        e.set_graph(self.s, self.r, self.N)
        if self.Fe2:
            e.set_edge_set(1, self.s2, self.r2)
            e.set_edge_features(1, self.ef2)
        e.set_trajectory(self.frames, dt=DT, node_type_onehot=self.onehot, ef_raw=self.ef_raw)
        return e


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


# ---- 1. two doors, one result --------------------------------------------------------------------------------------------------------
# L 64 (no fp16 pieces) and 128 (pieces, absmax on the device); hidden_layers 1 .. 4 (one- and two-block tables, identity slots); both
# ln_modes; a second edge set; whole-array LayerNorm; O in 1, 2, 3 (the decoder's O-wide bias in the T_B3 table, param_count % 4)
DOORS = {
    "L64": dict(L=64, hl=2, O=2),
    "L128-hl1-lnmode1-O1": dict(L=128, hl=1, O=1, ln_mode=1),
    "L128-hl2": dict(L=128, hl=2, O=2),
    "L128-hl3-O3": dict(L=128, hl=3, O=3),
    "L128-hl4-lnmode1": dict(L=128, hl=4, O=2, ln_mode=1),
    "L128-two-sets": dict(L=128, hl=2, O=2, Fe2=4),
    "L128-lnall-O3": dict(L=128, hl=2, O=3, ln_dims="all"),
}


def test_param_counts_are_not_all_multiples_of_four():
    rem = set()
    for c in DOORS.values():
        e = mgn_amd.Engine(c["O"] + NTYPES, FE, c["O"], c["L"], c["hl"], MPS, Fe2=c.get("Fe2"), device=mgn_amd.MGN_DEVICE_NONE)
        rem.add(e.param_count % 4)
        e.close()
    assert len(rem) >= 3 and rem != {0}, rem


@pytest.mark.parametrize("name", list(DOORS))
def test_two_doors_one_result(name):
    c = dict(DOORS[name])
    L, hl, O, Fe2 = c.pop("L"), c.pop("hl"), c.pop("O"), c.pop("Fe2", None)
    P = Problem(O, Fe2=Fe2)
    ps = P.params(L, hl)
    a, b = P.engine(L, hl, **c), P.engine(L, hl, **c)
    a.set_params(ps)
    b.set_params_dev(dev(ps))
    for run in (lambda e: e.step(P.nf, P.ef, P.target, P.mask), lambda e: e.step_datapoint(1, P.mask)):
        (ga, la), (gb, lb) = run(a), run(b)
        assert np.isfinite(la) and np.abs(ga).max() > 0
        assert la == lb
        assert same_bits(ga, gb)
    # and the other way round on the same handles: the host door after the device door, the device door (from host memory) after the host door
    ps2 = P.params(L, hl, seed=8)
    a.set_params_dev(ps2)
    b.set_params(ps2)
    (ga, la), (gb, lb) = a.step_datapoint(0, P.mask), b.step_datapoint(0, P.mask)
    assert la == lb and same_bits(ga, gb)
    assert same_bits(a.get_params(), ps2) and same_bits(b.get_params(), ps2)
    a.close()
    b.close()


# ---- 2. Adam bits --------------------------------------------------------------------------------------------------------------------
HYPER = dict(eta=1e-3, beta=(0.9, 0.999), epsilon=1e-8)


def plain_engine(**kw):
    """no graph: the parameter and optimiser calls need none.  16 321 parameters: one more than a multiple of four"""
    e = mgn_amd.Engine(4, 3, 1, 32, 2, 1, **kw)
    assert e.param_count % 4 == 1
    return e


def check_state(e, st, ps):
    got = e.adam_state()
    assert same_bits(e.get_params(), ps)
    assert same_bits(got["mt"], st["mt"]) and same_bits(got["vt"], st["vt"])
    assert got["beta_t"].dtype == np.float64 and np.array_equal(got["beta_t"], st["beta_t"])


@pytest.mark.parametrize("where", ["host", "device", "device-unaligned"])
def test_adam_bits(where):
    e = plain_engine()
    n = e.param_count
    ps = (np.random.default_rng(3).standard_normal(n) * 0.2).astype(F)
    e.set_params(ps)
    e.adam_init(**HYPER)
    st = adam_f32.setup(n, HYPER["beta"])
    check_state(e, st, ps)
    for k in range(3):
        g = adam_f32.synthetic_grads(n, 40 + k)
        assert (g == 0).sum() > 100 and np.abs(g).max() > 500 and np.abs(g[g != 0]).min() < 2e-3
        if where == "host":
            e.adam_update(g)
        elif where == "device":
            e.adam_update(dev(g))
        else:                                   # a view one float into a larger device array: not 16-byte aligned
            big = torch.zeros(n + 1, device="cuda")
            big[1:] = dev(g)
            torch.cuda.synchronize()            # (torch's stream filled it; the engine reads it on its own)
            e.adam_update(big[1:])
        st, ps = adam_f32.update(st, ps, g, **HYPER)
        check_state(e, st, ps)
    e.close()


def test_adam_on_a_rank_handle():
    """every rank of a partitioned mesh holds the whole vector: the calls do not ask about the partition"""
    e = plain_engine(rank=1, nranks=2)
    n = e.param_count
    ps = (np.random.default_rng(4).standard_normal(n) * 0.2).astype(F)
    e.set_params_dev(dev(ps))
    e.adam_init(**HYPER)
    g = adam_f32.synthetic_grads(n, 50)
    e.adam_update(dev(g))
    st, ps = adam_f32.update(adam_f32.setup(n, HYPER["beta"]), ps, g, **HYPER)
    check_state(e, st, ps)
    e.close()


# ---- 3. the loop ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cyl():
    return Problem(2, kind="cyl")


def test_loop_equivalence(cyl):
    """four iterations of step_datapoint(out = device) + adam_update against step_datapoint + the float32 restatement on the host +
    set_params: the same losses, the same final bits (mgn_step is bitwise repeatable where no mask entry repeats)"""
    P, L, hl = cyl, 128, 2
    ps = P.params(L, hl)
    a, b = P.engine(L, hl), P.engine(L, hl)
    a.set_params_dev(dev(ps))
    a.adam_init(**HYPER)
    b.set_params(ps)
    st = adam_f32.setup(ps.size, HYPER["beta"])
    gdev = torch.empty(ps.size, device="cuda")
    for k in range(4):
        t = k % (T - 1)
        _, la = a.step_datapoint(t, P.mask, out=gdev)
        a.adam_update(gdev)
        gb, lb = b.step_datapoint(t, P.mask)
        assert la == lb, (k, la, lb)
        st, ps = adam_f32.update(st, ps, gb, **HYPER)
        b.set_params(ps)
    assert same_bits(a.get_params(), ps)
    check_state(a, st, ps)
    a.close()
    b.close()


# ---- 4. every reader sees the update -------------------------------------------------------------------------------------------------
def test_every_reader_sees_the_update(cyl):
    P, L, hl = cyl, 128, 2
    ps0 = P.params(L, hl)
    e = P.engine(L, hl)
    e.set_params(ps0)
    x0 = P.frames[0]

    def readers(eng):
        out = eng.forward(P.nf, P.ef)
        sol, _ = eng.rollout("Euler", x0, P.onehot, P.ef_raw, 0.0, 0.05, 0.01, 6, dt=0.01)
        gs, loss, losses = eng.step_datapoints([0, 1], P.mask)
        return out, sol, gs, F(loss), losses

    # the layouts, the captured inference graphs and the companion exist BEFORE the update: all of them must follow it
    for _ in range(3):
        before = readers(e)
    e.adam_init(**HYPER)
    g, _ = e.step_datapoint(0, P.mask, out=torch.empty(ps0.size, device="cuda"))
    e.adam_update(g)
    ps1 = e.get_params()
    assert not same_bits(ps1, ps0)
    pdev = e.get_params(out=torch.empty(ps0.size, device="cuda"))
    e.synchronize()
    assert same_bits(pdev.cpu().numpy(), ps1)
    fresh = P.engine(L, hl)
    fresh.set_params(ps1)
    assert same_bits(fresh.get_params(), ps1)
    after, want = readers(e), readers(fresh)
    for got, ref, old in zip(after, want, before):
        assert same_bits(got, ref)
        assert not same_bits(got, old)
    # the stale-shortcut case: the values the HOST copy held before the update are new to the engine now
    e.set_params(ps0)
    assert same_bits(e.get_params(), ps0)
    back = readers(e)
    for got, old in zip(back, before):
        assert same_bits(got, old)
    e.close()
    fresh.close()


# ---- 5. state round trip -------------------------------------------------------------------------------------------------------------
def two_updates():
    e = plain_engine()
    n = e.param_count
    e.set_params((np.random.default_rng(5).standard_normal(n) * 0.2).astype(F))
    e.adam_init(**HYPER)
    for k in range(2):
        e.adam_update(adam_f32.synthetic_grads(n, 60 + k))
    return e, adam_f32.synthetic_grads(n, 62)


def test_state_round_trip():
    e, g3 = two_updates()
    st, ps = e.adam_state(), e.get_params()
    assert set(st) == {"mt", "vt", "beta_t"} and st["mt"].dtype == st["vt"].dtype == F and st["beta_t"].dtype == np.float64
    e2 = plain_engine()
    e2.set_params(ps)
    e2.adam_init(**HYPER)
    e2.set_adam_state(st)
    e.adam_update(g3)
    e2.adam_update(dev(g3))
    check_state(e2, e.adam_state(), e.get_params())
    e.close()
    e2.close()


def test_state_through_save_and_load(tmp_path):
    e, g3 = two_updates()

    class Holder:
        pass

    m = Holder()
    m.ps = e.get_params()
    m.e_norm, m.n_norm, m.o_norm = (ra.NormaliserOfflineMinMax(0.0, 1.0) for _ in range(3))
    eng_mod.save(m, e.adam_state(), ck.LossLog(), ck.LossLog(), 2, 0.5, str(tmp_path))
    norms = [ra.NormaliserOfflineMinMax(0.0, 1.0) for _ in range(3)]
    mgn, opt_state, df_train, _ = eng_mod.load(4, 2, norms[0], norms[1], norms[2], 1, 1, 32, 2, ck.Adam(**HYPER), None, str(tmp_path))
    assert df_train.step == [2] and set(opt_state) == {"mt", "vt", "beta_t"}
    e2 = mgn.engine
    e2.set_params_dev(mgn.ps)
    e2.adam_init(**HYPER)
    e2.set_adam_state(opt_state)
    e.adam_update(g3)
    e2.adam_update(g3)
    check_state(e2, e.adam_state(), e.get_params())
    e.close()
    e2.close()


def test_a_state_of_the_host_twin_is_accepted():
    e = plain_engine()
    n = e.param_count
    ps = (np.random.default_rng(6).standard_normal(n) * 0.2).astype(F)
    twin = ck.Adam(**HYPER)
    st, ps1 = twin.update(twin.setup(ps), ps, adam_f32.synthetic_grads(n, 70))
    e.set_params(ps1)
    e.adam_init(**HYPER)
    e.set_adam_state(st)
    check_state(e, st, ps1)
    g = adam_f32.synthetic_grads(n, 71)
    e.adam_update(g)                              # ... and the run goes on from it: the restatement from the same state
    st2, ps2 = adam_f32.update(st, ps1, g, **HYPER)
    check_state(e, st2, ps2)
    e.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------
def code_of(call):
    with pytest.raises(mgn_amd.MgnError) as ei:
        call()
    return ei.value.code


def test_refusals_leave_the_handle_usable():
    e = plain_engine()
    n = e.param_count
    lib, h = e.lib, e.h
    ps = (np.random.default_rng(8).standard_normal(n) * 0.2).astype(F)
    g = adam_f32.synthetic_grads(n, 80)
    gd, buf = dev(g), torch.empty(n, device="cuda")
    bt = np.zeros(2, np.float64)
    btp = bt.ctypes.data_as(_capi._f64p)
    p = _capi.f32(np.zeros(n + 1, F))
    STATE, ARG = _capi.MGN_E_STATE, _capi.MGN_E_ARG
    # before any parameters, before adam_init
    assert code_of(lambda: e.get_params(out=buf)) == STATE
    assert code_of(lambda: e.adam_update(gd)) == STATE
    assert code_of(e.adam_state) == STATE
    assert lib.mgn_adam_state(h, 1, p, p, btp) == STATE
    e.adam_init(**HYPER)
    assert code_of(lambda: e.adam_update(gd)) == STATE            # the optimiser exists, parameters do not
    e.set_params_dev(dev(ps))
    # arguments
    assert lib.mgn_adam_update(h, None, n) == ARG and lib.mgn_adam_update(h, p, n + 1) == ARG
    assert lib.mgn_set_params_dev(h, None, n) == ARG and lib.mgn_set_params_dev(h, p, n - 1) == ARG
    assert lib.mgn_get_params_dev(h, None, n) == ARG and lib.mgn_get_params_dev(h, p, n + 1) == ARG
    assert lib.mgn_adam_state(h, 2, p, p, btp) == ARG and lib.mgn_adam_state(h, 0, None, p, btp) == ARG
    assert lib.mgn_adam_init(h, None) == ARG
    for bad in (dict(eta=0.0), dict(eta=float("nan")), dict(beta=(1.0, 0.999)), dict(beta=(0.9, -0.1)), dict(epsilon=0.0),
                dict(epsilon=float("inf"))):
        assert code_of(lambda: e.adam_init(**dict(HYPER, **bad))) == ARG, bad
    # nothing of the above moved the state: the update from here is the first one on ps
    e.adam_update(gd)
    st, ps1 = adam_f32.update(adam_f32.setup(n, HYPER["beta"]), ps, g, **HYPER)
    check_state(e, st, ps1)
    # set_params* leave the optimiser's state alone; adam_init resets it
    e.set_params(ps)
    e.set_params_dev(dev(ps))
    check_state(e, st, ps)
    e.adam_init(**HYPER)
    check_state(e, adam_f32.setup(n, HYPER["beta"]), ps)
    e.close()


def test_a_new_graph_keeps_the_optimiser(cyl):
    P, L, hl = cyl, 64, 2
    e = P.engine(L, hl)
    ps = P.params(L, hl)
    e.set_params_dev(dev(ps))
    e.adam_init(**HYPER)
    g, _ = e.step_datapoint(0, P.mask, out=torch.empty(ps.size, device="cuda"))
    e.adam_update(g)
    st, ps1 = e.adam_state(), e.get_params()
    s, r = small_graph()
    e.set_graph(s, r, 70)
    check_state(e, st, ps1)
    e.close()
