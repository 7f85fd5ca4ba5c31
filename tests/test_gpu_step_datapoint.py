"""Derivative training on a device-resident trajectory (mgn_train_set_trajectory / mgn_step_datapoint and their kin): the loop
`for datapoint in 1:delta` of the reference's default strategy (src/MeshGraphNets.jl:364-378 over src/strategies.jl:395-416) with
the trajectory, the noise and the online normalisers on the device.

Checked against (1) the existing path bit for bit -- the exported datapoint fed to Engine.step -- (2) the NumPy mirror
reference_api.init_train_step_derivative, (3) the float64 oracle, and for the noise and the online normalisers against their
definitions.  Shapes: util.small_mesh(8, 6) (48 nodes: two node tiles, the second ragged), O = 2, three node types (Fn = 5), Fe = 3,
mps = 2, T = 4, L in {32, 128}, hidden_layers 2 and once 3, once two edge sets.

"ulp" below, for a value of an affine map y = x * scale + shift, is the spacing of float32 at the largest of |x * scale|, |shift| and
|y|: the magnitude the map rounds at.  The device evaluates the product form (possibly as one FMA), the mirror (x - mean) / std; both
round at that magnitude, and where x is close to the mean the result itself is smaller than the rounding of its terms."""
import ctypes as C

import numpy as np
import pytest
import torch   # noqa: F401  (before the engine's first HIP call)

import mgn_amd
import mgn_oracle as orc
from mgn_amd import reference_api as ra
from mgn_amd import synth
from mgn_amd._capi import f32, i32
from train_checks import affine_ulps
from util import rel_max, renumbered, scatter_labels, set_renumber, small_mesh

pytestmark = pytest.mark.gpu

F32 = np.float32
O, NTYPES, FN, FE, T, MPS = 2, 3, 5, 3, 4, 2
TOL_GRAD, TOL_LOSS = 1e-3, 1e-4      # as tests/test_gpu_training_general.py holds mgn_step to at these shapes: relative L2, relative
DT = F32(0.01)
TIMES = np.array([0.0, 0.01, 0.035, 0.04], F32)      # unequal steps

CASES = [pytest.param(32, 2, None, id="L32"), pytest.param(128, 2, None, id="L128"), pytest.param(128, 3, None, id="L128-hl3"),
         pytest.param(128, 2, 4, id="L128-two-sets")]


def cfg_of(L, hl=2, Fe2=None):
    c = dict(Fn=FN, Fe=FE, O=O, L=L, hidden_layers=hl, mps=MPS)
    if Fe2:
        c["Fe2"] = Fe2
    return c


def params_of(cfg, seed=7):
    return orc.init_params(cfg["Fn"], cfg["Fe"], cfg["O"], cfg["L"], cfg["hidden_layers"], cfg["mps"], seed, 0.1, Fe2=cfg.get("Fe2"))


def engine_of(cfg, **kw):
    return mgn_amd.Engine(cfg["Fn"], cfg["Fe"], cfg["O"], cfg["L"], cfg["hidden_layers"], cfg["mps"], Fe2=cfg.get("Fe2"), **kw)


class Mgn:
    """What init_train_step / build_graph read of the reference's GraphNetwork: the normalisers."""

    def __init__(self, n_norm, e_norm, o_norm):
        self.n_norm, self.e_norm, self.o_norm = n_norm, e_norm, o_norm


class Problem:
    def __init__(self):
        self.pos, self.s, self.r = small_mesh(8, 6)
        self.N, self.E = self.pos.shape[0], self.s.size
        rng = np.random.default_rng(5)
        N, E = self.N, self.E
        self.frames = (rng.standard_normal((T, N, O)) * np.array([1.5, 0.3]) + np.array([2.0, -0.5])).astype(F32)
        self.types = rng.integers(0, NTYPES, N)
        self.onehot = ra.one_hot(self.types, NTYPES)
        self.ef_raw = (rng.standard_normal((E, FE)) * np.array([0.2, 0.2, 0.1]) + np.array([0.0, 0.1, 0.3])).astype(F32)
        self.mask = np.sort(rng.choice(N, int(0.6 * N), replace=False)).astype(np.int32)
        # a second edge set (world edges) for the two-set case: its features go in as for mgn_step
        self.s2, self.r2 = synth.random_graph(N, 40, 9)
        self.ef2 = rng.standard_normal((self.s2.size, 4)).astype(F32)
        self.stddev = np.array([0.02, 0.05], F32)
        self.noisy = (self.types != 1)
        self.frozen = Mgn({"velocity": ra.NormaliserOfflineMeanStd(np.array([1.9, -0.4], F32), np.array([1.4, 0.33], F32)),
                           "node_type": ra.NormaliserOfflineMinMax(0.0, 1.0)},
                          ra.NormaliserOfflineMeanStd(np.array([0.01, 0.09, 0.31], F32), np.array([0.21, 0.19, 0.11], F32)),
                          {"velocity": ra.NormaliserOfflineMeanStd(np.array([0.7, -3.0], F32), np.array([140.0, 35.0], F32))})
        # add_targets! (reference src/dataset.jl:461-481): the field without its last frame, the target without its first
        self.data = {"velocity": self.frames[:-1], "target|velocity": self.frames[1:]}

    def norms(self, mgn=None):
        mgn = mgn or self.frozen
        vs, vsh = mgn.n_norm["velocity"].affine(O)
        ts, tsh = mgn.n_norm["node_type"].affine(NTYPES)
        return dict(node=(np.concatenate([vs, ts]), np.concatenate([vsh, tsh])), edge=mgn.e_norm.affine(FE),
                    out=mgn.o_norm["velocity"].inverse_affine(O))

    def mirror(self, t, meta, mgn=None, data=None):
        g, tq = ra.init_train_step_derivative(mgn or self.frozen, data or self.data, meta, ["velocity"], ["velocity"], self.onehot,
                                              self.ef_raw, self.s, self.r, t)
        return g.nf, g.ef, tq

    def engine(self, cfg, ps=None, frozen=True, times=None, **kw):
        eng = engine_of(cfg, **kw)
        if ps is not None:
            eng.set_params(ps)
        if frozen:
            eng.set_norms(**self.norms())
        eng.set_graph(self.s, self.r, self.N)
        if cfg.get("Fe2"):
            eng.set_edge_set(1, self.s2, self.r2)
            eng.set_edge_features(1, self.ef2)
        self.upload(eng, times)
        return eng

    def upload(self, eng, times=None):
        if times is None:
            eng.set_trajectory(self.frames, dt=DT, node_type_onehot=self.onehot, ef_raw=self.ef_raw)
        else:
            eng.set_trajectory(self.frames, times=times, node_type_onehot=self.onehot, ef_raw=self.ef_raw)

    def oracle(self, ps, cfg, nf, ef, tq):
        set2 = (self.ef2, self.s2, self.r2) if cfg.get("Fe2") else None
        return orc.step_grads(ps, cfg, nf, ef, self.s, self.r, tq, self.mask, set2=set2) if set2 else \
            orc.step_grads(ps, cfg, nf, ef, self.s, self.r, tq, self.mask)


@pytest.fixture(scope="module")
def prob():
    return Problem()


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def ulps(a, b):
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return float((np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(np.float64)).max())


def check_against_step(eng, mask, ts=(0, 1, T - 2)):
    """step_datapoint(t) == Engine.step on datapoint_export(t), bit for bit; returns the results of the last t."""
    for t in ts:
        nf, ef, tq = eng.datapoint_export(t)
        gs_a, loss_a = eng.step(nf, ef, tq, mask)
        gs_b, loss_b = eng.step_datapoint(t, mask)
        assert np.isfinite(loss_b) and np.abs(gs_b).max() > 0
        assert loss_a == loss_b and same_bits(gs_a, gs_b), (t, loss_a, loss_b)
        gs_c, loss_c = eng.step_datapoint(t, mask)           # again: the kept edge rows, the replayed launch graphs
        assert loss_c == loss_b and same_bits(gs_c, gs_b), t
    return gs_b.copy(), loss_b


# ---- 1. bits against the existing path ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,hl,Fe2", CASES)
def test_bits_against_step(prob, L, hl, Fe2):
    cfg = cfg_of(L, hl, Fe2)
    ps = params_of(cfg)
    eng = prob.engine(cfg, ps)
    gs0, loss0 = check_against_step(eng, prob.mask)
    # noise on
    eng.set_noise(prob.stddev, prob.noisy, seed=11)
    gs1, loss1 = check_against_step(eng, prob.mask)
    assert loss1 != loss0 and not same_bits(gs1, gs0)
    # new parameters between the calls (what a training loop does before every step): the trajectory and the noise survive
    nf_before = eng.datapoint_export(T - 2)
    ps2 = params_of(cfg, seed=8)
    eng.set_params(ps2)
    gs2, loss2 = eng.step_datapoint(T - 2, prob.mask)
    assert loss2 != loss1
    for a, b in zip(nf_before, eng.datapoint_export(T - 2)):
        assert same_bits(a, b)
    gs3, loss3 = eng.step(*nf_before, prob.mask)
    assert loss3 == loss2 and same_bits(gs3, gs2)
    eng.set_params(ps)
    gs4, loss4 = eng.step_datapoint(T - 2, prob.mask)
    assert loss4 == loss1 and same_bits(gs4, gs1)
    # set_norms keeps the trajectory too, and the kept edge rows follow the new norms
    eng.set_norms(node=prob.norms()["node"], edge=None, out=prob.norms()["out"])
    check_against_step(eng, prob.mask, ts=(1,))
    assert same_bits(eng.datapoint_export(1)[1], prob.ef_raw)


def test_bits_on_a_scattered_numbering(prob):
    cfg = cfg_of(128)
    ps = params_of(cfg)
    pos2, s2, r2, perm = scatter_labels(prob.pos, prob.s, prob.r, seed=2)
    inv = np.argsort(perm)
    frames, onehot, noisy = np.ascontiguousarray(prob.frames[:, inv]), prob.onehot[inv], prob.noisy[inv]
    mask = np.sort(perm[prob.mask]).astype(np.int32)
    engines = []
    old = set_renumber(0)
    try:
        for mode in (0, 2):
            set_renumber(mode)
            eng = engine_of(cfg)
            eng.set_params(ps)
            eng.set_norms(**prob.norms())
            eng.set_graph(s2, r2, prob.N)
            assert renumbered(eng) == (mode == 2)
            eng.set_trajectory(frames, times=TIMES, node_type_onehot=onehot, ef_raw=prob.ef_raw)
            engines.append(eng)
    finally:
        set_renumber(old)
    plain, renum = engines
    for noise in (False, True):
        for eng in engines:
            eng.set_noise(prob.stddev if noise else None, noisy, seed=3)
        check_against_step(renum, mask)
        for t in range(T - 1):
            for normalised in (True, False):
                for a, b in zip(plain.datapoint_export(t, normalised), renum.datapoint_export(t, normalised)):
                    assert same_bits(a, b), (noise, t, normalised)
        # the same mesh under the scattered labels is the same problem: the loss of the unscattered engine to rounding (noise off)
        if not noise:
            want = prob.engine(cfg, ps, times=TIMES).step_datapoint(1, prob.mask)[1]
            assert abs(want - renum.step_datapoint(1, mask)[1]) <= 1e-5 * abs(want)
    cur = renum.datapoint_export(0, normalised=False)[0][:, :O]
    assert np.array_equal(cur[~noisy], frames[0][~noisy]) and not np.array_equal(cur[noisy], frames[0][noisy])


# ---- 2. assembly against the host mirror ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("times", [None, TIMES], ids=["dt", "times"])
def test_assembly_against_the_mirror(prob, times):
    cfg = cfg_of(32)
    eng = prob.engine(cfg, times=times)
    meta = {"dt": float(DT) if times is None else times}
    nrm = prob.norms()
    shift, scale = nrm["out"][1], nrm["out"][0]
    for t in range(T - 1):
        delta = DT if times is None else F32(times[t + 1] - times[t])
        nf, ef, tq = eng.datapoint_export(t)
        rnf, ref_, d = eng.datapoint_export(t, normalised=False)
        cur, nxt = prob.frames[t], prob.frames[t + 1]
        d_np = ((nxt - cur) / F32(delta)).astype(F32)
        assert same_bits(rnf, np.concatenate([cur, prob.onehot], 1)) and same_bits(ref_, prob.ef_raw)
        assert same_bits(d, d_np)
        assert same_bits(tq, ((d_np - shift) / scale).astype(F32))
        mnf, mef, mtq = prob.mirror(t, meta)
        assert same_bits(tq, mtq)
        u_nf = affine_ulps(nf, mnf, rnf, nrm["node"][0], nrm["node"][1])
        u_ef = affine_ulps(ef, mef, ref_, nrm["edge"][0], nrm["edge"][1])
        print(f"t={t}: nf {u_nf:.2f} ulp, ef {u_ef:.2f} ulp against build_graph")
        assert u_nf <= 2.0 and u_ef <= 2.0, (u_nf, u_ef)
        assert np.array_equal(nf[:, O:], prob.onehot)               # (the reference's min-max normaliser of node_type over [0, 1])


# ---- 3. against the oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,hl,Fe2", CASES)
def test_against_the_oracle(prob, L, hl, Fe2):
    cfg = cfg_of(L, hl, Fe2)
    ps = params_of(cfg)
    eng = prob.engine(cfg, ps, times=TIMES)
    for t in (0, T - 2):
        gs, loss = eng.step_datapoint(t, prob.mask)
        nf, ef, tq = prob.mirror(t, {"dt": TIMES})
        ref, ref_loss = prob.oracle(ps, cfg, nf, ef, tq)
        gerr = float(np.linalg.norm(gs - ref) / np.linalg.norm(ref))
        print(f"t={t}: loss {loss} vs {ref_loss}, gradient rel L2 {gerr:.2e}")
        assert abs(loss - ref_loss) <= TOL_LOSS * abs(ref_loss), (loss, ref_loss)
        assert gerr <= TOL_GRAD, gerr


# ---- 4. noise -------------------------------------------------------------------------------------------------------------------
def test_noise_rows_target_and_seeds(prob):
    eng = prob.engine(cfg_of(32), frozen=False)
    clean = [eng.datapoint_export(t, normalised=False) for t in range(T - 1)]
    big = np.array([1e4, 0.05], F32)                           # huge on one column: any of it inside frames[t + 1] would show
    eng.set_noise(big, prob.noisy, seed=21)
    raw = [eng.datapoint_export(t, normalised=False) for t in range(T - 1)]
    for t in range(T - 1):
        cur, d = raw[t][0][:, :O], raw[t][2]
        assert same_bits(cur[~prob.noisy], prob.frames[t][~prob.noisy])
        assert same_bits(d[~prob.noisy], clean[t][2][~prob.noisy])
        assert np.all(cur[prob.noisy] != prob.frames[t][prob.noisy])
        assert same_bits(raw[t][0][:, O:], prob.onehot) and same_bits(raw[t][1], prob.ef_raw)
        # d Delta + cur gives the clean next frame back: the difference and the quotient were rounded once each
        back = d.astype(np.float64) * float(DT) + cur.astype(np.float64)
        nxt = prob.frames[t + 1]
        bound = 2.0 * np.spacing(np.abs(nxt) + np.abs(cur)).astype(np.float64)
        assert np.all(np.abs(back - nxt) <= bound), float((np.abs(back - nxt) / bound).max())
    # the same seed gives the same bits; another seed, another datapoint give other values
    again = eng.datapoint_export(1, normalised=False)
    assert all(same_bits(a, b) for a, b in zip(again, raw[1]))
    z = [(raw[t][0][:, :O].astype(np.float64) - prob.frames[t]) / big for t in range(T - 1)]
    assert np.abs(z[0] - z[1])[prob.noisy].min() > 0 and np.abs(z[1] - z[2])[prob.noisy].min() > 0
    eng.set_noise(big, prob.noisy, seed=22)
    other = eng.datapoint_export(1, normalised=False)[0][:, :O]
    assert np.all(other[prob.noisy] != raw[1][0][:, :O][prob.noisy])
    eng.set_noise(big, None, seed=21)                              # every node; the noisy ones keep their values
    allnodes = eng.datapoint_export(1, normalised=False)[0][:, :O]
    assert same_bits(allnodes[prob.noisy], raw[1][0][:, :O][prob.noisy]) and np.all(allnodes != prob.frames[1])
    eng.set_noise()
    assert all(same_bits(a, b) for a, b in zip(eng.datapoint_export(1, normalised=False), clean[1]))


@pytest.mark.parametrize("seed", [1, 2])
def test_noise_is_standard_normal(seed):
    pos, cells = synth.grid_mesh(50, 40, 1)
    s, r = synth.cells_to_edges(cells)
    N = pos.shape[0]
    assert N == 2000
    rng = np.random.default_rng(0)
    frames = rng.standard_normal((T, N, O)).astype(F32)
    stddev = np.array([0.5, 3.0], F32)
    eng = mgn_amd.Engine(O, FE, O, 32, 2, MPS)
    eng.set_graph(s, r, N)
    eng.set_trajectory(frames, dt=DT, ef_raw=np.zeros((s.size, FE), F32))
    eng.set_noise(stddev, None, seed=seed)
    z = np.concatenate([(eng.datapoint_export(t, normalised=False)[0].astype(np.float64) - frames[t]) / stddev for t in range(T - 1)]).ravel()
    n = z.size
    assert n == (T - 1) * N * O
    print(f"seed {seed}: mean {z.mean():+.4f} (band {5 / np.sqrt(n):.4f}), std - 1 {z.std() - 1:+.4f} (band {5 / np.sqrt(2 * n):.4f})")
    assert abs(z.mean()) <= 5 / np.sqrt(n)
    assert abs(z.std() - 1) <= 5 / np.sqrt(2 * n)
    for col in range(O):                                           # and per column, the bands of its own sample count
        zc = z.reshape(-1, O)[:, col]
        assert abs(zc.mean()) <= 5 / np.sqrt(zc.size) and abs(zc.std() - 1) <= 5 / np.sqrt(2 * zc.size)


# ---- 5. online normalisers ------------------------------------------------------------------------------------------------------
PROBE = F32(2.0 ** 40)


def read_maps(eng, prob):
    """The affine maps as the device holds them, through the normalised export of a probe trajectory: x = 0 gives the shift, x = 2^40
    gives 2^40 scale exactly (the shift is below half an ulp of it); for the output d = 0 gives (0 - mean) / std and d = 2^40 gives
    2^40 / std = 2^40 (1.0f / std).  The real trajectory is put back afterwards.  Returns node (scale, shift), edge (scale, shift) and
    the output's (1 / std, -mean / std)."""
    N, E = prob.N, prob.E
    frames = np.zeros((2, N, O), F32)
    frames[1, 1::3] = PROBE
    frames[0, 2::3] = PROBE
    ef = np.zeros((E, FE), F32)
    ef[1::2] = PROBE
    eng.set_trajectory(frames, dt=1.0, node_type_onehot=prob.onehot, ef_raw=ef)
    nf, efn, tq = eng.datapoint_export(0)
    prob.upload(eng)
    for a in (nf[0::3, :O], nf[2::3, :O], efn[0::2], efn[1::2], tq[0::3], tq[1::3]):
        assert np.all(a == a[0])
    return ((nf[2, :O] / PROBE, nf[0, :O]), (efn[1] / PROBE, efn[0]), (tq[1] / PROBE, tq[0]))


def test_online_normalisers(prob):
    cfg = cfg_of(32)
    ps = params_of(cfg)
    N, E = prob.N, prob.E
    eng = prob.engine(cfg, ps)                          # frozen maps first: the one-hot columns keep theirs
    eng.online_norms(max_acc=1e6, std_epsilon=1e-8)
    on_n, on_e, on_o = ra.NormaliserOnline(O), ra.NormaliserOnline(FE), ra.NormaliserOnline(O)
    for on in (on_n, on_e, on_o):
        on.engine = eng                                 # (its float64 totals through mgn_feature_stats, as the class offers)
    mgn = Mgn({"velocity": on_n, "node_type": prob.frozen.n_norm["node_type"]}, on_e, {"velocity": on_o})
    tot = [[np.zeros(d), np.zeros(d)] for d in (O, FE, O)]
    states = []
    for k, t in enumerate((0, 1, 2)):
        rnf, ref_, d = eng.datapoint_export(t, normalised=False)
        raws = (np.ascontiguousarray(rnf[:, :O]), ref_, d)
        for g in range(3):
            s_, q_ = eng.feature_stats(raws[g])
            tot[g][0] += s_
            tot[g][1] += q_
        gs, loss = eng.step_datapoint(t, prob.mask, accumulate=True)
        for g, rows in enumerate((N, E, N)):
            s_, q_, count, calls = eng.norm_state(g)
            assert np.array_equal(s_, tot[g][0]) and np.array_equal(q_, tot[g][1]), (t, g)
            assert count == (k + 1) * rows and calls == k + 1
        states.append([eng.norm_state(g) for g in range(3)])
        # the mirror: NormaliserOnline called on the same raw arrays accumulates, then normalises
        mnf, mef, mtq = prob.mirror(t, {"dt": float(DT)}, mgn)
        nf, ef, tq = eng.datapoint_export(t)
        (ns, nsh), (es, esh), (os_, osh) = read_maps(eng, prob)
        fn, fe, fo = on_n.frozen(), on_e.frozen(), on_o.frozen()
        u = (affine_ulps(nf[:, :O], mnf[:, :O], raws[0], *fn.affine(O)), affine_ulps(ef, mef, raws[1], *fe.affine(FE)),
             affine_ulps(tq, mtq, raws[2], *fo.affine(O)))
        um = (ulps(ns, fn.affine(O)[0]), ulps(nsh, fn.affine(O)[1]), ulps(es, fe.affine(FE)[0]), ulps(esh, fe.affine(FE)[1]),
              ulps(os_, F32(1.0) / fo.std), ulps(osh, (-fo.mean / fo.std).astype(F32)))
        ref, ref_loss = prob.oracle(ps, cfg, mnf, mef, mtq)
        gerr = float(np.linalg.norm(gs - ref) / np.linalg.norm(ref))
        print(f"t={t}: arrays {u} ulp, maps {um} ulp, loss {loss} vs {ref_loss}, gradient rel L2 {gerr:.2e}")
        assert max(u) <= 2.0, u
        assert max(um) <= 1.0, um
        assert np.array_equal(nf[:, O:], prob.onehot)
        assert abs(loss - ref_loss) <= TOL_LOSS * abs(ref_loss) and gerr <= TOL_GRAD, (loss, ref_loss, gerr)
        # the step consumed what the export shows
        gs_s, loss_s = eng.step(nf, ef, tq, prob.mask)
        assert loss_s == loss and same_bits(gs_s, gs)
    gs_last, loss_last = gs.copy(), loss
    # without `accumulate` the maps are used as they stand
    before = [eng.norm_state(g) for g in range(3)]
    gs_n, loss_n = eng.step_datapoint(2, prob.mask)
    assert loss_n == loss_last and same_bits(gs_n, gs_last)
    assert all(np.array_equal(a[0], b[0]) and a[2:] == b[2:] for a, b in zip(before, [eng.norm_state(g) for g in range(3)]))
    # restored totals reproduce the next step's bits (the checkpoint hook): back to the state after two calls, then the third
    eng.online_norms()
    assert all(eng.norm_state(g)[2:] == (0.0, 0.0) and not eng.norm_state(g)[0].any() for g in range(3))
    for g in range(3):
        eng.set_norm_state(g, *states[1][g])
    gs_r, loss_r = eng.step_datapoint(2, prob.mask, accumulate=True)
    assert loss_r == loss_last and same_bits(gs_r, gs_last)
    for g in range(3):
        a, b = eng.norm_state(g), states[2][g]
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2:] == b[2:]
    # max_acc = 2: the third call leaves the totals alone
    eng.online_norms(max_acc=2)
    for k, t in enumerate((0, 1, 2)):
        eng.step_datapoint(t, prob.mask, accumulate=True)
        if k == 1:
            two = [eng.norm_state(g) for g in range(3)]
    for g in range(3):
        a = eng.norm_state(g)
        assert np.array_equal(a[0], two[g][0]) and np.array_equal(a[1], two[g][1]) and a[2:] == two[g][2:] and a[3] == 2.0
        assert np.array_equal(a[0], states[1][g][0])
    # a group left off keeps what set_norms gave it
    eng.set_norms(**prob.norms())
    eng.online_norms(node=False, edge=True, out=False)
    eng.step_datapoint(0, prob.mask, accumulate=True)
    nf, ef, tq = eng.datapoint_export(0)
    fnf, _, ftq = prob.engine(cfg, ps).datapoint_export(0)
    assert same_bits(nf, fnf) and same_bits(tq, ftq)
    assert eng.norm_state(1)[2:] == (float(E), 1.0) and eng.norm_state(0)[2:] == two[0][2:]      # (the edge group began anew, the others stand still)


@pytest.mark.parametrize("ln_dims", [0, 1], ids=["ln-rows", "ln-all"])
def test_later_entry_points_see_the_updated_norms(prob, ln_dims):
    """mgn_ode_step after an accumulating step computes with the rewritten maps: it agrees with an engine given the same maps
    through set_norms.  ln_dims = MGN_LN_ALL builds its inputs on the host, from the host copy of the norms."""
    cfg = cfg_of(32)
    ps = params_of(cfg)
    eng = prob.engine(cfg, ps, ln_dims=ln_dims)
    x = prob.frames[1]
    before = eng.ode_step(x, prob.onehot, prob.ef_raw)
    eng.online_norms()
    eng.step_datapoint(0, prob.mask, accumulate=True)
    after = eng.ode_step(x, prob.onehot, prob.ef_raw)
    assert rel_max(after, before) > 1e-2
    rnf, ref_, d = eng.datapoint_export(0, normalised=False)
    on_n, on_e, on_o = ra.NormaliserOnline(O), ra.NormaliserOnline(FE), ra.NormaliserOnline(O)
    for on, a in ((on_n, rnf[:, :O]), (on_e, ref_), (on_o, d)):
        on(a)
    mgn = Mgn({"velocity": on_n, "node_type": prob.frozen.n_norm["node_type"]}, on_e, {"velocity": on_o})
    other = engine_of(cfg, ln_dims=ln_dims)
    other.set_params(ps)
    other.set_norms(**prob.norms(mgn))
    other.set_graph(prob.s, prob.r, prob.N)
    want = other.ode_step(x, prob.onehot, prob.ef_raw)
    err = rel_max(after, want)
    print(f"ln_dims={ln_dims}: ode_step against set_norms with the same maps: {err:.2e}")
    assert err <= 1e-5


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------
def code_of(call):
    with pytest.raises(mgn_amd.MgnError) as ei:
        call()
    return ei.value.code


def test_refusals(prob):
    cfg = cfg_of(32)
    ps = params_of(cfg)
    N, E = prob.N, prob.E
    STATE, ARG = -3, -1
    eng = engine_of(cfg)
    eng.set_params(ps)
    # no graph
    assert code_of(lambda: eng.set_trajectory(np.zeros((T, 0, O), F32), dt=DT, node_type_onehot=np.zeros((0, NTYPES), F32),
                                              ef_raw=np.zeros((0, FE), F32))) == STATE
    assert code_of(lambda: eng.step_datapoint(0, prob.mask)) == STATE
    assert code_of(lambda: eng.datapoint_export(0)) == STATE
    eng.set_graph(prob.s, prob.r, N)
    # no trajectory
    assert code_of(lambda: eng.step_datapoint(0, prob.mask)) == STATE
    assert code_of(lambda: eng.datapoint_export(0)) == STATE
    prob.upload(eng)
    good = eng.step_datapoint(0, prob.mask)

    def still_good():
        gs, loss = eng.step_datapoint(0, prob.mask)
        assert loss == good[1] and same_bits(gs, good[0])

    kw = dict(node_type_onehot=prob.onehot, ef_raw=prob.ef_raw)
    bad_times = np.array([0.0, 0.01, 0.01, 0.02], F32)
    loss = C.c_float()
    buf = np.zeros(eng.param_count, F32)
    refused = [
        (lambda: eng.step_datapoint(-1, prob.mask), ARG),
        (lambda: eng.step_datapoint(T - 1, prob.mask), ARG),
        (lambda: eng.datapoint_export(T - 1), ARG),
        (lambda: eng.step_datapoint(0, np.zeros(0, np.int32)), ARG),                          # mgn_step's own checks
        (lambda: eng.step_datapoint(0, np.array([N], np.int32)), ARG),
        (lambda: eng.step_datapoint(0, np.array([0], np.int32), mask_index_base=1), ARG),
        (lambda: eng.step_datapoint(0, prob.mask, mask_index_base=2), ARG),
        (lambda: eng._chk(eng.lib.mgn_step_datapoint(eng.h, 0, 0, i32(prob.mask), prob.mask.size, 0, f32(buf), buf.size - 1, C.byref(loss))), ARG),
        (lambda: eng._chk(eng.lib.mgn_step_datapoint(eng.h, 0, 0, None, prob.mask.size, 0, f32(buf), buf.size, C.byref(loss))), ARG),
        (lambda: eng.online_norms(max_acc=0), ARG),
        (lambda: eng.online_norms(std_epsilon=0.0), ARG),
        (lambda: eng.norm_state(3), ARG),
        (lambda: eng.norm_state(-1), ARG),
        (lambda: eng.set_norm_state(3, np.zeros(1), np.zeros(1), 0, 0), ARG),
    ]
    for call, want in refused:
        assert code_of(call) == want
        still_good()
    # refusals at upload: the handle stays usable, a valid upload and step follow
    uploads = [
        (lambda: eng.set_trajectory(prob.frames[:1], dt=DT, **kw), ARG),                        # T < 2
        (lambda: eng.set_trajectory(prob.frames, dt=DT, ef_raw=prob.ef_raw), ARG),              # onehot missing, Fn > O
        (lambda: eng.set_trajectory(prob.frames, dt=DT, node_type_onehot=prob.onehot), ARG),    # ef_raw missing, E > 0
        (lambda: eng.set_trajectory(prob.frames, times=bad_times, **kw), ARG),                  # a zero time step
        (lambda: eng.set_trajectory(prob.frames, dt=0.0, **kw), ARG),
    ]
    for call, want in uploads:
        assert code_of(call) == want
        prob.upload(eng)
        still_good()
    # a new graph drops the trajectory
    eng.set_graph(prob.s, prob.r, N)
    assert code_of(lambda: eng.step_datapoint(0, prob.mask)) == STATE
    prob.upload(eng)
    still_good()
    # Fn < O
    narrow = mgn_amd.Engine(1, FE, O, 32, 2, MPS)
    narrow.set_graph(prob.s, prob.r, N)
    assert code_of(lambda: narrow.set_trajectory(prob.frames, dt=DT, ef_raw=prob.ef_raw)) == ARG
    narrow.set_graph(prob.s, prob.r, N)
    # a partitioned handle, a bf16 handle
    part = mgn_amd.Engine(FN, FE, O, 32, 2, MPS, rank=0, nranks=2)
    part.set_graph(prob.s, prob.r, N)
    half = mgn_amd.Engine(FN, FE, O, 128, 2, MPS, dtype="bf16")
    half.set_graph(prob.s, prob.r, N)
    for e in (part, half):
        assert code_of(lambda: e.set_trajectory(prob.frames, dt=DT, **kw)) == STATE
        assert code_of(lambda: e.set_noise(prob.stddev)) == STATE
        assert code_of(lambda: e.online_norms()) == STATE
        assert code_of(lambda: e.norm_state(0)) == STATE
        assert code_of(lambda: e.step_datapoint(0, prob.mask)) == STATE
        assert code_of(lambda: e.datapoint_export(0)) == STATE
        e.set_graph(prob.s, prob.r, N)
