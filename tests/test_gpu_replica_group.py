"""Replica groups (mgn_group_create_replicas, mgn_group_step_datapoints) and the group forms of Adam and the resident parameters
(mgn_group_set_params_dev / get_params_dev / adam_init / adam_update / adam_state), on replica groups and on a partition group.

The problem is tests/test_gpu_step_datapoint.py's: the 8 x 6 mesh (N = 48, E = 234), noise on a subset of the nodes, frozen norms,
unequal time steps, T = 4 (datapoints 0 .. 2).  All ranks run on device 0; P is 2 or 3.

Checked (1) bit for bit against the definition: the NumPy float64 fold -- s = 0.0, then s = s + (B_k / B) * g_k over the replicas
with a share in ascending order, every product and sum rounded once, the result rounded to float32 -- of the plain Engine's
step_datapoints / step_datapoint results on the same shares, the losses those calls' bits, the loss the documented host expression;
(2) against one handle's step_datapoints on the whole list (the replicas sum in another grouping: the loop-against-batch bounds
SEQ_LOSS / SEQ_GRAD of tests/test_gpu_step_datapoints.py) and against the float64 oracle's mean (TOL_LOSS / TOL_GRAD of
tests/test_gpu_step_datapoint.py); (3) that the replicas stay in step over three iterations of step_datapoints(want_grads=False) +
adam_update() with accumulating online normalisers, bit-equal to a plain Engine fed the host-folded gradients; (4) repeatability;
(5) a partition group: B = 1 is mgn_group_step_datapoint's bits, Adam keeps the ranks bit-equal, B = 2 is MGN_E_STATE;
(6) the refusals, each leaving the group usable, and a failure behind the checks on one replica alone, after which nobody waits in
the gather.

Measured on an MI355X (test 2; nothing is asserted from these):
  L32   P2 len 3: loss rel 0.00e+00 vs one handle, gradient rel L2 1.85e-07; oracle: loss rel 3.88e-08, gradient rel L2 1.81e-07
  L128  P2 len 3: loss rel 0.00e+00 vs one handle, gradient rel L2 1.57e-07; oracle: loss rel 4.59e-10, gradient rel L2 2.23e-07
(bounds: SEQ_LOSS 1e-5, SEQ_GRAD 1e-4 against one handle; TOL_LOSS 1e-4, TOL_GRAD 1e-3 against the oracle)
Run on the MI355X box with `-m gpu`."""
import functools

import numpy as np
import pytest
import torch   # noqa: F401  (before the engine's first HIP call)

from mgn_amd import GroupEngine, MgnError
from mgn_amd._capi import MGN_E_ARG, MGN_E_OOM, MGN_E_STATE, MGN_E_UNSUPPORTED
from test_gpu_step_datapoint import T, TIMES, TOL_GRAD, TOL_LOSS, Problem, cfg_of, code_of, params_of, same_bits
from test_gpu_step_datapoints import SEQ_GRAD, SEQ_LOSS, rel, rel_l2

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SEED = 11
LS = [pytest.param(32, id="L32"), pytest.param(128, id="L128")]
# (P, list): shares 2 + 1 (companion path and single path), 3 + 2 (two companion sizes), 1 + 1 + 0 (an idle replica)
SHAPES = [pytest.param(2, (2, 0, 1), id="P2-len3"), pytest.param(2, (2, 0, 1, 1, 0), id="P2-len5"), pytest.param(3, (1, 2), id="P3-len2")]


def shares(B, P):
    """[(first, count)] per replica: contiguous chunks in listed order"""
    q, r = divmod(B, P)
    return [(k * q + min(k, r), q + (1 if k < r else 0)) for k in range(P)]


def host_loss(losses):
    s = 0.0
    for v in losses:
        s += float(v)
    return F32(s / len(losses))


def definition(eng, ts, P, mask):
    """(gradient, loss, losses) of the replica group's call by its definition, from the plain engine's results on the shares"""
    B = len(ts)
    s = np.zeros(eng.param_count, F64)
    losses = np.zeros(B, F32)
    for first, count in shares(B, P):
        if count == 0:
            continue
        chunk = list(ts[first:first + count])
        if count == 1:
            g, l1 = eng.step_datapoint(chunk[0], mask)
            ls = [l1]
        else:
            g, _, ls = eng.step_datapoints(chunk, mask)
        losses[first:first + count] = ls
        w = F64(count) / F64(B)
        prod = w * g.astype(F64)
        s = s + prod
    return s.astype(F32), host_loss(losses), losses


def make_group(prob, cfg, ps, P, replicas=True, **kw):
    g = GroupEngine(cfg["Fn"], cfg["Fe"], cfg["O"], cfg["L"], cfg["hidden_layers"], cfg["mps"], devices=[0] * P, replicas=replicas, **kw)
    g.set_params(ps)
    g.set_norms(**prob.norms())
    g.set_graph(prob.s, prob.r, prob.N, mesh_pos=None if replicas else prob.pos)
    g.set_trajectory(prob.frames, times=TIMES, node_type_onehot=prob.onehot, ef_raw=prob.ef_raw)
    g.set_noise(prob.stddev, prob.noisy, seed=SEED)
    return g


def make_plain(prob, cfg, ps, **kw):
    e = prob.engine(cfg, ps, times=TIMES, **kw)
    e.set_noise(prob.stddev, prob.noisy, seed=SEED)
    return e


@functools.lru_cache(maxsize=None)
def case(L):
    """The plain engine of a case and its replica groups by P: made once, shared by the tests that leave their state alone."""
    prob = Problem()
    cfg = cfg_of(L)
    ps = params_of(cfg)
    return dict(prob=prob, cfg=cfg, ps=ps, plain=make_plain(prob, cfg, ps), groups={})


def group_of(L, P):
    c = case(L)
    if P not in c["groups"]:
        c["groups"][P] = make_group(c["prob"], c["cfg"], c["ps"], P)
    return c["groups"][P]


@functools.lru_cache(maxsize=None)
def defined(L, P, ts):
    c = case(L)
    g, loss, losses = definition(c["plain"], ts, P, c["prob"].mask)
    for a in (g, losses):
        a.setflags(write=False)
    return g, loss, losses


def test_the_split_rule():
    assert shares(3, 2) == [(0, 2), (2, 1)] and shares(5, 2) == [(0, 3), (3, 2)] and shares(2, 3) == [(0, 1), (1, 1), (2, 0)]


# ---- 1. bits against the definition ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,ts", SHAPES)
@pytest.mark.parametrize("L", LS)
def test_bits_against_the_definition(L, P, ts):
    c = case(L)
    grp = group_of(L, P)
    want_g, want_loss, want_losses = defined(L, P, ts)
    gs, loss, losses = grp.step_datapoints(ts, c["prob"].mask)
    assert np.isfinite(loss) and np.abs(gs).max() > 0
    print(f"gradient bits equal: {same_bits(gs, want_g)} (rel L2 {rel_l2(gs, want_g.astype(F64)):.2e}); loss {loss} vs {want_loss}")
    assert same_bits(gs, want_g)
    assert same_bits(losses, want_losses)
    assert F32(loss) == want_loss
    # nothing downloaded: the same losses, and the resident gradient is the one Adam reads (test 3)
    none, loss2, losses2 = grp.step_datapoints(ts, c["prob"].mask, want_grads=False)
    assert none is None and loss2 == loss and same_bits(losses2, losses)


# ---- 2. the same model as one handle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", LS)
def test_same_model_as_one_handle(L):
    c = case(L)
    prob, plain = c["prob"], c["plain"]
    P, ts = 2, (2, 0, 1)
    gs, loss, losses = group_of(L, P).step_datapoints(ts, prob.mask)
    one_g, one_loss, one_losses = plain.step_datapoints(ts, prob.mask)
    gerr = rel_l2(gs, one_g.astype(F64))
    print(f"loss {loss} vs one handle {one_loss} (rel {rel(loss, one_loss):.2e}), gradient rel L2 {gerr:.2e}")
    refs = [prob.oracle(c["ps"], c["cfg"], *plain.datapoint_export(t)) for t in ts]
    ref_g = np.mean([np.asarray(g, F64) for g, _ in refs], axis=0)
    ref_loss = float(np.mean([F64(l) for _, l in refs]))
    oerr = rel_l2(gs, ref_g)
    print(f"oracle: loss rel {rel(loss, ref_loss):.2e}, gradient rel L2 {oerr:.2e}")
    assert rel(loss, one_loss) <= SEQ_LOSS and gerr <= SEQ_GRAD
    assert rel(loss, ref_loss) <= TOL_LOSS and oerr <= TOL_GRAD
    for b, (_, l) in enumerate(refs):
        assert rel(losses[b], l) <= TOL_LOSS


# ---- 3. the replicas stay in step ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,P", [pytest.param(32, 2, id="L32-P2"), pytest.param(128, 2, id="L128-P2"), pytest.param(32, 3, id="L32-P3")])
def test_replicas_stay_in_step(L, P):
    c = case(L)
    prob, cfg, ps = c["prob"], c["cfg"], c["ps"]
    plain = make_plain(prob, cfg, ps)
    grp = make_group(prob, cfg, ps, P)
    try:
        for e in (plain, grp):
            e.online_norms(node=True, edge=False, out=True, max_acc=1e6, std_epsilon=1e-8)
            e.adam_init(eta=1e-3)
        grp.set_params_dev(ps)
        for ts in ((2, 0, 1), (1, 0, 2, 2, 1), (0, 1)):
            none, loss, losses = grp.step_datapoints(ts, prob.mask, accumulate=True, want_grads=False)
            assert none is None
            grp.adam_update()
            plain.step_datapoints(ts, prob.mask, accumulate=True)          # the accumulations of the whole list, in listed order
            want_g, want_loss, want_losses = definition(plain, ts, P, prob.mask)
            assert F32(loss) == want_loss and same_bits(losses, want_losses)
            plain.adam_update(want_g)
            want_p = plain.get_params()
            got = [grp.get_params_dev(k) for k in range(P)]
            for k in range(P):
                assert same_bits(got[k], got[0]), k
            print(f"list {ts}: parameters bit-equal to the plain engine: {same_bits(got[0], want_p)}")
            assert same_bits(got[0], want_p)
            assert not same_bits(got[0], ps)
        for g in range(3):
            a, b = plain.norm_state(g), grp.norm_state(g)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2:] == b[2:], g
        assert grp.norm_state(0)[3] == 10.0 and grp.norm_state(1)[3] == 0.0
        sa, sb = plain.adam_state(), grp.adam_state()
        assert same_bits(sa["mt"], sb["mt"]) and same_bits(sa["vt"], sb["vt"]) and np.array_equal(sa["beta_t"], sb["beta_t"])
    finally:
        grp.close()
        plain.close()


# ---- 4. repeatable ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,ts", [pytest.param(2, (2, 0, 1), id="P2"), pytest.param(3, (1, 2), id="P3")])
@pytest.mark.parametrize("L", LS)
def test_repeatable(L, P, ts):
    c = case(L)
    grp = group_of(L, P)
    a = grp.step_datapoints(ts, c["prob"].mask)
    a = (a[0].copy(), a[1], a[2].copy())
    b = grp.step_datapoints(ts, c["prob"].mask)
    assert b[1] == a[1] and same_bits(b[0], a[0]) and same_bits(b[2], a[2])


# ---- 5. a partition group --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", LS)
def test_partition_group(L):
    c = case(L)
    prob, cfg, ps = c["prob"], c["cfg"], c["ps"]
    grp = make_group(prob, cfg, ps, 2, replicas=False)
    plain = make_plain(prob, cfg, ps)
    try:
        want = grp.step_datapoint(1, prob.mask)
        want = (want[0].copy(), want[1])
        gs, loss, losses = grp.step_datapoints([1], prob.mask)
        assert loss == want[1] and same_bits(gs, want[0]) and losses.shape == (1,) and losses[0] == F32(loss)
        assert code_of(lambda: grp.step_datapoints((1, 0), prob.mask)) == MGN_E_STATE
        again = grp.step_datapoints([1], prob.mask, want_grads=False)
        assert again[0] is None and again[1] == loss
        for e in (grp, plain):
            e.adam_init(eta=1e-3)
        grp.adam_update()
        plain.adam_update(gs)
        p0, p1 = grp.get_params_dev(0), grp.get_params_dev(1)
        assert same_bits(p0, p1) and same_bits(p0, plain.get_params()) and not same_bits(p0, ps)
        after = grp.step_datapoints([1], prob.mask)                      # the group steps on, with the new parameters
        assert np.isfinite(after[1]) and after[1] != loss
    finally:
        grp.close()
        plain.close()


# ---- 6. refusals, and a failure behind the checks ----------------------------------------------------------------------------------
def test_one_replica_failing_behind_the_checks(monkeypatch):
    """Behind the checks one replica alone fails -- its companion's arena is refused (MGN_TRAIN_TEST_FAIL_ALLOCS, the hook of
    tests/test_gpu_step_datapoints.py) -- while the other, whose share of one needs no new arena, succeeds: the call ends with the
    first failure's status before anyone enters the gather, nobody waits, and the next call works on a fresh communicator."""
    monkeypatch.setenv("MGN_COMM_TIMEOUT_S", "20")                       # (read when the communicator is made: a wait nobody answers ends the test)
    c = case(32)
    prob, cfg, ps = c["prob"], c["cfg"], c["ps"]
    grp = make_group(prob, cfg, ps, 2)
    try:
        first = grp.step_datapoints((2, 1), prob.mask)                   # shares 1 + 1: both replicas build their own arenas
        assert same_bits(first[0], defined(32, 2, (2, 1))[0])
        monkeypatch.setenv("MGN_TRAIN_TEST_FAIL_ALLOCS", "3")
        with pytest.raises(MgnError) as ei:
            grp.step_datapoints((2, 0, 1), prob.mask)                    # shares 2 + 1: replica 0 needs a companion of two copies
        monkeypatch.delenv("MGN_TRAIN_TEST_FAIL_ALLOCS")
        assert ei.value.code == MGN_E_OOM and "rank 0" in str(ei.value), str(ei.value)
        assert code_of(lambda: grp.adam_update()) == MGN_E_STATE           # the failed call left no gradient to apply
        gs, loss, losses = grp.step_datapoints((2, 0, 1), prob.mask)
        want = defined(32, 2, (2, 0, 1))
        assert same_bits(gs, want[0]) and F32(loss) == want[1] and same_bits(losses, want[2])
    finally:
        grp.close()


def test_refusals():
    c = case(32)
    prob, cfg, ps = c["prob"], c["cfg"], c["ps"]
    ts = (2, 0, 1)
    grp = make_group(prob, cfg, ps, 2)
    try:
        grp.adam_init()
        assert code_of(lambda: grp.adam_update()) == MGN_E_STATE           # no group step yet
        good = grp.step_datapoints(ts, prob.mask)
        good = (good[0].copy(), good[1], good[2].copy())
        assert same_bits(good[0], defined(32, 2, ts)[0])

        def still_good():
            gs, loss, losses = grp.step_datapoints(ts, prob.mask)
            assert loss == good[1] and same_bits(gs, good[0]) and same_bits(losses, good[2])

        refused = [
            (lambda: grp.step_datapoints((0, T - 1, 1), prob.mask), MGN_E_ARG),                          # a datapoint out of range
            (lambda: grp.step_datapoints((0, -1), prob.mask), MGN_E_ARG),
            (lambda: grp.step_datapoints(ts, prob.mask, out=np.zeros(grp.param_count - 1, F32)), MGN_E_ARG),   # a wrong n_grads
            (lambda: grp.step_datapoints(ts, np.zeros(0, np.int32)), MGN_E_ARG),                         # an empty mask
            (lambda: grp.step_datapoints(ts, np.array([prob.N], np.int32)), MGN_E_ARG),
            (lambda: grp.step_datapoints(ts, prob.mask, mask_index_base=2), MGN_E_ARG),
            (lambda: grp.step_datapoints([], prob.mask), MGN_E_ARG),
            (lambda: grp.step_datapoints([i % (T - 1) for i in range(130)], prob.mask), MGN_E_ARG),      # a share of 65
            (lambda: grp.get_params_dev(2), MGN_E_ARG),
            (lambda: grp.adam_update(np.zeros(grp.param_count - 1, F32)), MGN_E_ARG),
        ]
        for k, (call, want) in enumerate(refused):
            assert code_of(call) == want, k
            still_good()
    finally:
        grp.close()
    # whole-array LayerNorm on a replica group: legal, and the rule of the call is the rule of its largest share
    lnall = make_group(prob, cfg, ps, 2, ln_dims="all")
    plain = make_plain(prob, cfg, ps, ln_dims="all")
    try:
        assert code_of(lambda: lnall.step_datapoints((2, 0, 1), prob.mask)) == MGN_E_UNSUPPORTED      # shares 2 + 1
        want_g, want_loss, want_losses = definition(plain, (2, 1), 2, prob.mask)                       # shares 1 + 1
        gs, loss, losses = lnall.step_datapoints((2, 1), prob.mask)
        assert same_bits(gs, want_g) and F32(loss) == want_loss and same_bits(losses, want_losses)
    finally:
        lnall.close()
        plain.close()
