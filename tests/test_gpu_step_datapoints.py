"""mgn_step_datapoints: step! on the block-diagonal FeatureGraph of B datapoints of the resident trajectory (the reference's
Args.batchsize, src/MeshGraphNets.jl:39,224, for the loop of src/MeshGraphNets.jl:364-378).

Checked (1) bit for bit against a second engine that is given the union graph of the B copies, the concatenated exports and the
replicated mask through Engine.step, (2) against the float64 mean of the oracle's step over the exported datapoints, (3) on a
renumbered parent against the float64 mean of sequential step_datapoint calls, (4) across the size regimes of the training step (one copy
on the cooperative kernels, four copies on the eight-tile streaming ones), (5) for the online normalisers' totals, (6) for what the call
leaves of the handle's state -- a new trajectory and an mgn_shooting_grad call on the same companion included --, (7) for its refusals.  The problem is tests/test_gpu_step_datapoint.py's: the 8 x 6 mesh (N = 48, E = 234),
noise on a subset of the nodes, frozen norms, unequal time steps.

Bounds.  TOL_GRAD / TOL_LOSS: test_gpu_step_datapoint.py's against the oracle.  SEQ_LOSS / SEQ_GRAD: the loop-against-batch bounds of
tests/test_gpu_shooting_batched.py (the same model on B times the rows may run other kernels and other partial sums).  Against the
union engine the gradient is held to equal bits: both run the same launches on the same rows; the loss to 1e-6 relative -- the union
folds B nmask terms' block partials on the host in another grouping than the per-copy slots, plus one float rounding of the result."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch   # noqa: F401  (before the engine's first HIP call)

import mgn_amd
import mgn_oracle as orc
from mgn_amd import reference_api as ra
from mgn_amd._capi import MGN_E_ARG, MGN_E_OOM, MGN_E_STATE, MGN_E_UNSUPPORTED, f32, i32
from test_gpu_step_datapoint import (FE, FN, MPS, NTYPES, O, T, TIMES, TOL_GRAD, TOL_LOSS, Problem, cfg_of, code_of, engine_of, params_of,
                                     same_bits)
from util import renumbered, scatter_labels, set_num_cus, set_renumber, small_mesh, train_regime

pytestmark = pytest.mark.gpu

F32 = np.float32
SEQ_LOSS, SEQ_GRAD = 1e-5, 1e-4
CASES = [pytest.param(32, 2, id="L32"), pytest.param(128, 2, id="L128"), pytest.param(128, 3, id="L128-hl3")]
TS = (T - 2, 0, 1)


@pytest.fixture(scope="module")
def prob():
    return Problem()


def rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


def rel_l2(a, ref):
    return float(np.linalg.norm(np.asarray(a, np.float64) - ref) / np.linalg.norm(ref))


def union_graph(s, r, N, B):
    return (np.concatenate([s + w * N for w in range(B)]).astype(np.int32), np.concatenate([r + w * N for w in range(B)]).astype(np.int32))


def sequential_mean(eng, ts, mask):
    """float64 mean of step_datapoint over ts (each distinct datapoint run once): (gradient, loss, the single results by datapoint)"""
    single = {t: eng.step_datapoint(t, mask) for t in sorted(set(ts))}
    g = np.mean([single[t][0].astype(np.float64) for t in ts], axis=0)
    return g, float(np.mean([np.float64(single[t][1]) for t in ts])), single


@functools.lru_cache(maxsize=None)
def case(L, hl):
    """One engine per case with noise on and unequal time steps, its batched result on TS, and the references every test of the case
    shares: computed once, left unchanged."""
    prob = Problem()
    cfg = cfg_of(L, hl)
    ps = params_of(cfg)
    old = set_renumber(0)
    try:
        eng = prob.engine(cfg, ps, times=TIMES)
        union = engine_of(cfg)
        union.set_params(ps)
        union.set_graph(*union_graph(prob.s, prob.r, prob.N, len(TS)), len(TS) * prob.N)
    finally:
        set_renumber(old)
    assert not renumbered(eng) and not renumbered(union)
    eng.set_noise(prob.stddev, prob.noisy, seed=11)
    exports = [eng.datapoint_export(t) for t in TS]
    batched = eng.step_datapoints(TS, prob.mask)
    return dict(prob=prob, cfg=cfg, ps=ps, eng=eng, union=union, exports=exports, batched=(batched[0].copy(), batched[1], batched[2].copy()))


# ---- 1. bits against the union graph through Engine.step -------------------------------------------------------------------------
@pytest.mark.parametrize("L,hl", CASES)
def test_bits_against_the_union_graph(L, hl):
    c = case(L, hl)
    prob, eng, union = c["prob"], c["eng"], c["union"]
    B, N = len(TS), prob.N
    gs, loss, losses = c["batched"]
    nf = np.concatenate([e[0] for e in c["exports"]])
    ef = np.concatenate([e[1] for e in c["exports"]])
    tq = np.concatenate([e[2] for e in c["exports"]])
    mask = np.concatenate([prob.mask + w * N for w in range(B)]).astype(np.int32)
    gs_u, loss_u = union.step(nf, ef, tq, mask)
    assert np.isfinite(loss) and np.abs(gs).max() > 0
    print(f"loss {loss} vs union {loss_u} (rel {rel(loss, loss_u):.2e}); gradient bits equal: {same_bits(gs, gs_u)}, "
          f"rel L2 {rel_l2(gs, gs_u.astype(np.float64)):.2e}")
    assert same_bits(gs, gs_u)
    assert rel(loss, loss_u) <= 1e-6
    singles = {t: eng.step_datapoint(t, prob.mask) for t in set(TS)}
    for b, t in enumerate(TS):
        print(f"losses[{b}] {losses[b]} vs step_datapoint({t}) {singles[t][1]}")
        assert rel(losses[b], singles[t][1]) <= 1e-5
    assert rel(loss, np.mean(losses.astype(np.float64))) <= 1e-6
    gs2, loss2, losses2 = eng.step_datapoints(TS, prob.mask)             # again: the kept edge rows, the replayed launch graphs
    assert loss2 == loss and same_bits(gs2, gs) and same_bits(losses2, losses)
    gs3, loss3, losses3 = eng.step_datapoints(TS, prob.mask)
    assert loss3 == loss and same_bits(gs3, gs) and same_bits(losses3, losses)
    for t in (0, T - 2):                                                  # B = 1 is step_datapoint
        g1, l1, ls1 = eng.step_datapoints([t], prob.mask)
        assert l1 == singles[t][1] and same_bits(g1, singles[t][0]) and ls1.shape == (1,) and ls1[0] == F32(l1)


# ---- 2. against the oracle ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,hl", CASES)
def test_against_the_oracle(L, hl):
    c = case(L, hl)
    prob = c["prob"]
    gs, loss, losses = c["batched"]
    refs = [prob.oracle(c["ps"], c["cfg"], *e) for e in c["exports"]]
    ref_g = np.mean([np.asarray(g, np.float64) for g, _ in refs], axis=0)
    ref_loss = float(np.mean([np.float64(l) for _, l in refs]))
    gerr = rel_l2(gs, ref_g)
    print(f"loss {loss} vs {ref_loss} (rel {rel(loss, ref_loss):.2e}), gradient rel L2 {gerr:.2e}")
    assert rel(loss, ref_loss) <= TOL_LOSS
    assert gerr <= TOL_GRAD
    for b, (_, l) in enumerate(refs):
        assert rel(losses[b], l) <= TOL_LOSS


# ---- 3. a renumbered parent, a datapoint listed twice ------------------------------------------------------------------------------
def test_scattered_labels_and_a_repeat(prob):
    cfg = cfg_of(128)
    ps = params_of(cfg)
    pos2, s2, r2, perm = scatter_labels(prob.pos, prob.s, prob.r, seed=2)
    inv = np.argsort(perm)
    frames, onehot, noisy = np.ascontiguousarray(prob.frames[:, inv]), prob.onehot[inv], prob.noisy[inv]
    mask = np.sort(perm[prob.mask]).astype(np.int32)
    old = set_renumber(2)
    try:
        eng = engine_of(cfg)
        eng.set_params(ps)
        eng.set_norms(**prob.norms())
        eng.set_graph(s2, r2, prob.N)
    finally:
        set_renumber(old)
    assert renumbered(eng)
    eng.set_trajectory(frames, times=TIMES, node_type_onehot=onehot, ef_raw=prob.ef_raw)
    eng.set_noise(prob.stddev, noisy, seed=3)
    ts = (1, 0, 1, 2)
    ref_g, ref_loss, single = sequential_mean(eng, ts, mask)
    gs, loss, losses = eng.step_datapoints(ts, mask)
    gerr = rel_l2(gs, ref_g)
    print(f"loss {loss} vs sequential mean {ref_loss} (rel {rel(loss, ref_loss):.2e}), gradient rel L2 {gerr:.2e}")
    assert rel(loss, ref_loss) <= SEQ_LOSS and gerr <= SEQ_GRAD
    print(f"the repeated datapoint's losses: {losses[0]} and {losses[2]}")
    assert rel(losses[0], losses[2]) <= SEQ_LOSS                          # the same datapoint, the same noise, another copy
    for b, t in enumerate(ts):
        assert rel(losses[b], single[t][1]) <= SEQ_LOSS
    gs1, loss1, _ = eng.step_datapoints(ts, mask + 1, mask_index_base=1)  # 1-based mask: the same entries
    assert loss1 == loss and same_bits(gs1, gs)


# ---- 4. one copy cooperative, four copies streaming --------------------------------------------------------------------------------
def test_regime_crossing():
    """16 x 12 grid, L = 128, mps = 2, under a test CU count of 8 (cooperative up to 64 tiles): one copy is 33 edge tiles, B = 4 is 131
    (eight-tile streaming kernels, aggregation inside the launch, LayerNorm sums in the backward kernel), B = 6 is 6252 edge rows
    (above the 6144-row weight-gradient rule).  Whole-gradient bounds only."""
    pos, s, r = small_mesh(16, 12)
    N, E = pos.shape[0], s.size
    assert (N, E) == (192, 1042)
    cfg = dict(Fn=FN, Fe=FE, O=O, L=128, hidden_layers=2, mps=2)
    ps = params_of(cfg, seed=9)
    rng = np.random.default_rng(17)
    frames = (rng.standard_normal((T, N, O)) * np.array([1.5, 0.3]) + np.array([2.0, -0.5])).astype(F32)
    onehot = ra.one_hot(rng.integers(0, NTYPES, N), NTYPES)
    ef_raw = (rng.standard_normal((E, FE)) * np.array([0.2, 0.2, 0.1]) + np.array([0.0, 0.1, 0.3])).astype(F32)
    mask = np.sort(rng.choice(N, int(0.6 * N), replace=False)).astype(np.int32)
    norms = Problem().norms()
    rc = set_num_cus(8)
    if rc != 0:
        if rc > 0:
            set_num_cus(rc)
        raise AssertionError(f"mgn_debug_num_cus(8) returned {rc}: an override was active, or this one was refused")
    try:
        eng = engine_of(cfg)
        try:
            eng.set_params(ps)
            eng.set_norms(**norms)
            eng.set_graph(s, r, N)
            eng.set_trajectory(frames, times=TIMES, node_type_onehot=onehot, ef_raw=ef_raw)
            eng.set_noise(np.array([0.02, 0.05], F32), None, seed=5)
            train_regime(None, reset=True)
            first = eng.step_datapoint(0, mask)
            one = train_regime(eng, reset=True)
            assert one["fwd"][0] > 0 and one["fwd"][2] == 0 and one["bwd"][2] == 0 and one["lin2"][2] == 0, one
            ts4, ts6 = (0, 1, 2, 0), (2, 1, 0, 0, 1, 2)
            res4 = eng.step_datapoints(ts4, mask)
            four = train_regime(None, reset=True)
            assert four["fwd"][2] > 0 and four["bwd"][2] > 0, four
            res4 = (res4[0].copy(), res4[1], res4[2].copy())
            res6 = eng.step_datapoints(ts6, mask)
            six = train_regime(None, reset=True)
            assert six["fwd"][2] > 0 and six["bwd"][2] > 0, six
            res6 = (res6[0].copy(), res6[1], res6[2].copy())
            again = eng.step_datapoints(ts4, mask)
            assert again[1] == res4[1] and same_bits(again[0], res4[0]) and same_bits(again[2], res4[2])
            single = {t: eng.step_datapoint(t, mask) for t in (0, 1, 2)}
            assert single[0][1] == first[1] and same_bits(single[0][0], first[0])
            exports = {t: eng.datapoint_export(t) for t in (0, 1, 2)}
        finally:
            eng.close()
    finally:
        set_num_cus(0)
    oracle = {t: orc.step_grads(ps, cfg, exports[t][0], exports[t][1], s, r, exports[t][2], mask) for t in (0, 1, 2)}
    for name, ts, (gs, loss, losses) in (("B=4", ts4, res4), ("B=6", ts6, res6)):
        ref_g = np.mean([np.asarray(oracle[t][0], np.float64) for t in ts], axis=0)
        ref_loss = float(np.mean([np.float64(oracle[t][1]) for t in ts]))
        seq_g = np.mean([single[t][0].astype(np.float64) for t in ts], axis=0)
        seq_loss = float(np.mean([np.float64(single[t][1]) for t in ts]))
        print(f"{name}: oracle loss rel {rel(loss, ref_loss):.2e} grad rel L2 {rel_l2(gs, ref_g):.2e}; "
              f"sequential loss rel {rel(loss, seq_loss):.2e} grad rel L2 {rel_l2(gs, seq_g):.2e}")
        assert rel(loss, ref_loss) <= TOL_LOSS and rel_l2(gs, ref_g) <= TOL_GRAD
        assert rel(loss, seq_loss) <= SEQ_LOSS and rel_l2(gs, seq_g) <= SEQ_GRAD
        assert rel(loss, np.mean(losses.astype(np.float64))) <= 1e-6


# ---- 5. online normalisers ---------------------------------------------------------------------------------------------------------
def test_online_normalisers_accumulate_first(prob):
    cfg = cfg_of(32)
    ps = params_of(cfg)
    ts = (0, 1, 2)
    seq, bat = prob.engine(cfg, ps), prob.engine(cfg, ps)
    for e in (seq, bat):
        e.online_norms(max_acc=1e6, std_epsilon=1e-8)
    for t in ts:
        last = seq.step_datapoint(t, prob.mask, accumulate=True)
    gs, loss, losses = bat.step_datapoints(ts, prob.mask, accumulate=True)
    gs, losses = gs.copy(), losses.copy()
    for g, rows in enumerate((prob.N, prob.E, prob.N)):
        a, b = seq.norm_state(g), bat.norm_state(g)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2:] == b[2:] == (3.0 * rows, 3.0), g
    # the last datapoint saw the same maps in both: all three accumulations
    assert rel(losses[2], last[1]) <= SEQ_LOSS
    # without `accumulate` the maps are used as they stand: the accumulating call's bits
    gs_n, loss_n, losses_n = bat.step_datapoints(ts, prob.mask)
    assert loss_n == loss and same_bits(gs_n, gs) and same_bits(losses_n, losses)
    for g in range(3):
        assert bat.norm_state(g)[2:] == seq.norm_state(g)[2:]
    # ... and they are the maps a sequential step without `accumulate` reads
    ref_g, ref_loss, _ = sequential_mean(seq, ts, prob.mask)
    assert rel(loss, ref_loss) <= SEQ_LOSS and rel_l2(gs, ref_g) <= SEQ_GRAD
    # max_acc = 2 and B = 3: the third datapoint leaves the totals alone
    seq.online_norms(max_acc=2)
    bat.online_norms(max_acc=2)
    for t in ts:
        seq.step_datapoint(t, prob.mask, accumulate=True)
    bat.step_datapoints(ts, prob.mask, accumulate=True)
    for g, rows in enumerate((prob.N, prob.E, prob.N)):
        a, b = seq.norm_state(g), bat.norm_state(g)
        assert b[3] == 2.0 and b[2] == 2.0 * rows
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


# ---- 6. what the call leaves of the handle's state ---------------------------------------------------------------------------------
def test_state(prob):
    cfg = cfg_of(128)
    ps = params_of(cfg)
    eng = prob.engine(cfg, ps, times=TIMES)
    eng.set_noise(prob.stddev, prob.noisy, seed=11)
    before = eng.step_datapoint(1, prob.mask)
    before = (before[0].copy(), before[1])
    ts = (2, 0)
    a = eng.step_datapoints(ts, prob.mask)
    a = (a[0].copy(), a[1], a[2].copy())
    after = eng.step_datapoint(1, prob.mask)
    assert after[1] == before[1] and same_bits(after[0], before[0])
    eng.set_params(params_of(cfg, seed=8))
    b = eng.step_datapoints(ts, prob.mask)
    assert b[1] != a[1] and not same_bits(b[0], a[0])
    eng.set_params(ps)
    c = eng.step_datapoints(ts, prob.mask)
    assert c[1] == a[1] and same_bits(c[0], a[0]) and same_bits(c[2], a[2])
    # new norms: the kept edge rows follow them
    eng.set_norms(node=prob.norms()["node"], edge=None, out=prob.norms()["out"])
    ref_g, ref_loss, _ = sequential_mean(eng, ts, prob.mask)
    d = eng.step_datapoints(ts, prob.mask)
    assert d[1] != a[1]
    assert rel(d[1], ref_loss) <= SEQ_LOSS and rel_l2(d[0], ref_g) <= SEQ_GRAD
    eng.set_norms(**prob.norms())
    # the largest batch: 64 copies of the 48-node mesh
    ts64 = [i % (T - 1) for i in range(64)]
    ref_g, ref_loss, single = sequential_mean(eng, ts64, prob.mask)
    gs, loss, losses = eng.step_datapoints(ts64, prob.mask)
    gerr = rel_l2(gs, ref_g)
    print(f"B = 64: loss {loss} vs sequential mean {ref_loss} (rel {rel(loss, ref_loss):.2e}), gradient rel L2 {gerr:.2e}")
    assert losses.shape == (64,)
    assert rel(loss, ref_loss) <= SEQ_LOSS and gerr <= SEQ_GRAD
    assert all(rel(losses[b], single[t][1]) <= SEQ_LOSS for b, t in enumerate(ts64))
    # a device tensor takes the gradient as in step()
    out = torch.zeros(eng.param_count, dtype=torch.float32, device="cuda")
    g_dev, loss_dev, _ = eng.step_datapoints(ts, prob.mask, out=out)
    torch.cuda.synchronize()
    assert loss_dev == a[1] and same_bits(out.cpu().numpy(), a[0])


def test_a_new_trajectory_renews_the_kept_edge_rows(prob):
    """set_trajectory with other edge features while the companion is alive: the replicated edge rows follow, and come back with the
    first trajectory."""
    cfg = cfg_of(128)
    ps = params_of(cfg)
    eng = prob.engine(cfg, ps, times=TIMES)
    ts = (2, 0)
    a = eng.step_datapoints(ts, prob.mask)
    a = (a[0].copy(), a[1], a[2].copy())
    other = np.ascontiguousarray(prob.ef_raw[::-1] * F32(1.5))
    eng.set_trajectory(prob.frames, times=TIMES, node_type_onehot=prob.onehot, ef_raw=other)
    ref_g, ref_loss, _ = sequential_mean(eng, ts, prob.mask)
    b = eng.step_datapoints(ts, prob.mask)
    print(f"other edge features: loss {b[1]} (first trajectory {a[1]}) vs sequential mean {ref_loss}, gradient rel L2 {rel_l2(b[0], ref_g):.2e}")
    assert b[1] != a[1]
    assert rel(b[1], ref_loss) <= SEQ_LOSS and rel_l2(b[0], ref_g) <= SEQ_GRAD
    prob.upload(eng, TIMES)
    c = eng.step_datapoints(ts, prob.mask)
    assert c[1] == a[1] and same_bits(c[0], a[0]) and same_bits(c[2], a[2])


def test_interleaved_with_shooting_grad_on_the_same_companion(prob):
    """mgn_shooting_grad solves B windows on the companion of B copies that step_datapoints(B) trains on, and its reverse sweep writes
    the call's own edge features into that companion's arena: the batched step must rebuild its edge rows afterwards.  Both orders --
    the companion created by the step (no inference latents, no norms: the solve brings them late) and created by the solve."""
    cfg = cfg_of(128)
    ps = params_of(cfg)
    ts = (2, 0)
    other = np.ascontiguousarray(prob.ef_raw[::-1] * F32(1.5))          # not the resident trajectory's edge features
    windows = [(0, 1), (1, 2)]                                          # two windows of one step each: one pass of B = 2

    def shoot(eng):
        t0s = [ra._range_at(0.0, 0.01, a, np.float32) for a, _ in windows]
        t1s = [ra._range_at(0.0, 0.01, b, np.float32) for _, b in windows]
        gs, loss = eng.shooting_grad(prob.onehot, other, prob.frames, windows, t0s, t1s, 0.01, 0.01, cont_weight=0.3)
        assert eng.last_shooting["n_groups"] == 1 and eng.last_shooting["n_passes"] == 1, eng.last_shooting
        return gs.copy(), loss

    first, second = prob.engine(cfg, ps, times=TIMES), prob.engine(cfg, ps, times=TIMES)
    # step, solve, step
    a = first.step_datapoints(ts, prob.mask)
    a = (a[0].copy(), a[1], a[2].copy())
    s1 = shoot(first)
    assert np.isfinite(s1[1]) and np.abs(s1[0]).max() > 0
    b = first.step_datapoints(ts, prob.mask)
    assert b[1] == a[1] and same_bits(b[0], a[0]) and same_bits(b[2], a[2])
    # solve, step, solve
    s2 = shoot(second)
    assert s2[1] == s1[1] and same_bits(s2[0], s1[0])                   # the late latents and norms of `first`'s companion served the solve
    c = second.step_datapoints(ts, prob.mask)
    assert c[1] == a[1] and same_bits(c[0], a[0]) and same_bits(c[2], a[2])
    s3 = shoot(second)
    assert s3[1] == s1[1] and same_bits(s3[0], s1[0])
    d = second.step_datapoints(ts, prob.mask)
    assert d[1] == a[1] and same_bits(d[0], a[0])
    ref_g, ref_loss, _ = sequential_mean(second, ts, prob.mask)
    assert rel(d[1], ref_loss) <= SEQ_LOSS and rel_l2(d[0], ref_g) <= SEQ_GRAD


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals(prob, monkeypatch):
    cfg = cfg_of(32)
    ps = params_of(cfg)
    N = prob.N
    eng = engine_of(cfg)
    eng.set_params(ps)
    ts = (0, 2)
    assert code_of(lambda: eng.step_datapoints(ts, prob.mask)) == MGN_E_STATE         # no graph
    eng.set_graph(prob.s, prob.r, N)
    assert code_of(lambda: eng.step_datapoints(ts, prob.mask)) == MGN_E_STATE         # no trajectory
    assert code_of(lambda: eng.step_datapoints([0], prob.mask)) == MGN_E_STATE
    prob.upload(eng)
    # the companion's arena does not fit: a clean MGN_E_OOM, and the next call builds it
    monkeypatch.setenv("MGN_TRAIN_TEST_FAIL_ALLOCS", "3")
    assert code_of(lambda: eng.step_datapoints(ts, prob.mask)) == MGN_E_OOM
    monkeypatch.delenv("MGN_TRAIN_TEST_FAIL_ALLOCS")
    good = eng.step_datapoints(ts, prob.mask)
    good = (good[0].copy(), good[1], good[2].copy())

    def still_good():
        gs, loss, losses = eng.step_datapoints(ts, prob.mask)
        assert loss == good[1] and same_bits(gs, good[0]) and same_bits(losses, good[2])

    loss = C.c_float()
    buf = np.zeros(eng.param_count, F32)
    ls = np.zeros(2, F32)
    dp = np.array(ts, np.int32)
    mk = prob.mask

    def raw(datapoints=dp, B=2, mask=mk, grads=buf, n_grads=None, loss_p=C.byref(loss)):
        n = buf.size if n_grads is None else n_grads
        return lambda: eng._chk(eng.lib.mgn_step_datapoints(eng.h, i32(datapoints) if datapoints is not None else None, B, 0,
                                                            i32(mask) if mask is not None else None, mk.size, 0,
                                                            f32(grads) if grads is not None else None, n, loss_p, f32(ls)))

    refused = [
        (raw(datapoints=None), MGN_E_ARG), (raw(mask=None), MGN_E_ARG), (raw(grads=None), MGN_E_ARG), (raw(loss_p=None), MGN_E_ARG),
        (raw(B=0), MGN_E_ARG), (raw(B=-1), MGN_E_ARG), (raw(B=65), MGN_E_ARG),
        (raw(n_grads=buf.size - 1), MGN_E_ARG), (raw(B=1, n_grads=buf.size - 1), MGN_E_ARG),
        (lambda: eng.step_datapoints([], prob.mask), MGN_E_ARG),
        (lambda: eng.step_datapoints(list(range(65)), prob.mask), MGN_E_ARG),
        (lambda: eng.step_datapoints((0, -1), prob.mask), MGN_E_ARG),
        (lambda: eng.step_datapoints((T - 1, 0), prob.mask), MGN_E_ARG),
        (lambda: eng.step_datapoints([T - 1], prob.mask), MGN_E_ARG),
        (lambda: eng.step_datapoints(ts, np.zeros(0, np.int32)), MGN_E_ARG),                      # mgn_step_datapoint's own checks
        (lambda: eng.step_datapoints(ts, np.array([N], np.int32)), MGN_E_ARG),
        (lambda: eng.step_datapoints(ts, np.array([0], np.int32), mask_index_base=1), MGN_E_ARG),
        (lambda: eng.step_datapoints(ts, prob.mask, mask_index_base=2), MGN_E_ARG),
    ]
    for k, (call, want) in enumerate(refused):
        assert code_of(call) == want, k
        still_good()
    # a new graph drops the trajectory and the companions
    eng.set_graph(prob.s, prob.r, N)
    assert code_of(lambda: eng.step_datapoints(ts, prob.mask)) == MGN_E_STATE
    prob.upload(eng)
    still_good()
    # two edge sets, whole-array LayerNorm: B = 1 is step_datapoint, B > 1 is refused
    for kw in (dict(Fe2=4), dict(ln_dims="all")):
        c2 = cfg_of(32, 2, kw.get("Fe2"))
        e2 = prob.engine(c2, params_of(c2), **({} if "Fe2" in kw else kw))
        want = e2.step_datapoint(1, prob.mask)
        want = (want[0].copy(), want[1])
        assert code_of(lambda: e2.step_datapoints((1, 0), prob.mask)) == MGN_E_UNSUPPORTED
        gs, loss1, losses = e2.step_datapoints([1], prob.mask)
        assert loss1 == want[1] and same_bits(gs, want[0]) and losses[0] == F32(loss1)
    # a partitioned handle, a bf16 handle: MGN_E_STATE.  What fires here is the datapoint family's common check -- no communicator on
    # the partitioned handle, dtype on the bf16 one -- before mgn_step_datapoints' own "B > 1 drives one partition" line, which only a
    # partitioned handle WITH a communicator and a trajectory reaches (more than one process: not covered here).  Neither handle can
    # make a successful call afterwards; set_graph shows it is usable.
    part = mgn_amd.Engine(FN, FE, O, 32, 2, MPS, rank=0, nranks=2)
    half = mgn_amd.Engine(FN, FE, O, 128, 2, MPS, dtype="bf16")
    for e in (part, half):
        e.set_graph(prob.s, prob.r, N)
        assert code_of(lambda: e.step_datapoints(ts, prob.mask)) == MGN_E_STATE
        e.set_graph(prob.s, prob.r, N)
