"""Derivative training on partitions: the datapoint family (mgn_train_set_trajectory, mgn_train_set_noise, mgn_train_online_norms,
mgn_train_norm_state, mgn_step_datapoint, mgn_datapoint_export) on rank handles with a communicator, and its group form
(mgn_group_train_* / mgn_group_step_datapoint / mgn_group_datapoint_export, GroupEngine).  Every rank is given the arrays of the whole
mesh, keeps the rows it owns, and returns the complete gradient and loss.

References: an unpartitioned Engine (exports bit for bit: the noise of a node does not depend on the partition), GroupEngine.step on
the exported arrays (bit for bit), thread-ranks over the "host" transport (bit for bit), the float64 oracle and the one-partition
step at the tolerances tests/test_gpu_partitioned_step.py holds mgn_step to, float64 NumPy sums for the online normalisers' totals.

Shapes: the 40 x 33 grid of grid_case (1320 nodes, L = 128, mps = 3, hidden_layers = 2; P = 2, 3, 4 on device 0, every rank has a
halo), T = 4 frames, O = 2, seven node types; once L = 32 with hidden_layers = 3 (the general kernels), once scattered labels (the
engine renumbers).  The staging buffer of the upload is cut to one and to two frames per pass in two of the cases.
Run on the MI355X box with `-m gpu`."""
import ctypes as C
import functools
import time

import numpy as np
import pytest
import torch   # noqa: F401  (before the engine's first HIP call)

import mgn_amd
import mgn_oracle as orc
from mgn_amd import GroupEngine, MgnError, _capi
from mgn_amd._capi import f32, i32
from test_gpu_partitioned_step import TOL_GRAD, TOL_LOSS, TOL_ORDER, check_grads, grid_case, rel_l2, run_ranks
from test_gpu_step_datapoint import read_maps, same_bits, ulps
from util import engine_for, renumbered, scatter_labels

pytestmark = pytest.mark.gpu

F32 = np.float32
T, SEED = 4, 11
TIMES = np.array([0.0, 0.01, 0.035, 0.04], F32)      # unequal steps
STATE, ARG, UNSUPPORTED = _capi.MGN_E_STATE, _capi.MGN_E_ARG, _capi.MGN_E_UNSUPPORTED

CASES = [pytest.param(2, 128, 2, False, 1, id="P2-one-frame-per-pass"), pytest.param(3, 128, 2, False, 25000, id="P3-two-frames-per-pass"),
         pytest.param(4, 128, 2, False, None, id="P4"), pytest.param(2, 32, 3, False, None, id="P2-L32-hl3"),
         pytest.param(2, 128, 2, True, None, id="P2-scattered")]


class Problem:
    """A trajectory on the grid of grid_case(L, 3, hl); scattered: the same mesh under arbitrary node labels."""

    def __init__(self, L, hl, scattered):
        self.cfg, pos, s, r, self.ps = grid_case(L, 3, hl)[:5]
        if scattered:
            pos, s, r, _ = scatter_labels(pos, s, r, seed=4)
        self.pos, self.s, self.r = pos, np.ascontiguousarray(s), np.ascontiguousarray(r)
        N, E = self.N, self.E = pos.shape[0], s.size
        O, Fn, Fe = self.cfg["O"], self.cfg["Fn"], self.cfg["Fe"]
        rng = np.random.default_rng(5)
        self.frames = (rng.standard_normal((T, N, O)) * np.array([1.5, 0.3]) + np.array([2.0, -0.5])).astype(F32)
        self.types = rng.integers(0, Fn - O, N)
        self.onehot = orc.one_hot(self.types, Fn - O, 0).astype(F32)
        self.ef_raw = (rng.standard_normal((E, Fe)) * np.array([0.2, 0.2, 0.1]) + np.array([0.0, 0.1, 0.3])).astype(F32)
        self.mask = np.sort(rng.choice(N, int(0.6 * N), replace=False)).astype(np.int32)
        self.stddev = np.array([0.02, 0.05], F32)
        self.noisy = self.types != 1
        vstd, vmean = np.array([1.4, 0.33], F32), np.array([1.9, -0.4], F32)
        estd, emean = np.array([0.21, 0.19, 0.11], F32), np.array([0.01, 0.09, 0.31], F32)
        ones, zeros = np.ones(Fn - O, F32), np.zeros(Fn - O, F32)
        self.norms = dict(node=(np.concatenate([1 / vstd, ones]), np.concatenate([-vmean / vstd, zeros])),
                          edge=(1 / estd, -emean / estd), out=(np.array([140.0, 35.0], F32), np.array([0.7, -3.0], F32)))

    def setup(self, e, norms=True):
        e.set_params(self.ps)
        if norms:
            e.set_norms(**self.norms)
        e.set_graph(self.s, self.r, self.N, mesh_pos=self.pos)

    def upload(self, e, noise=True):
        e.set_trajectory(self.frames, times=TIMES, node_type_onehot=self.onehot, ef_raw=self.ef_raw)
        if noise:
            e.set_noise(self.stddev, self.noisy, seed=SEED)

    def group(self, P, **kw):
        c = self.cfg
        return GroupEngine(c["Fn"], c["Fe"], c["O"], c["L"], c["hidden_layers"], c["mps"], devices=[0] * P, **kw)


@functools.lru_cache(maxsize=None)
def problem(L=128, hl=2, scattered=False):
    return Problem(L, hl, scattered)


@functools.lru_cache(maxsize=None)
def single(L=128, hl=2, scattered=False):
    """The unpartitioned handle's exports of every datapoint (normalised, raw), its steps on datapoints 0 and T - 2 and the oracle's
    step on the exported datapoint T - 2: computed once, shared, read-only.
    Why not datapoint 0: at L = 32, hidden_layers = 3 its float64 forward has the pre-activation of proc1_node, layer 3, node 1226,
    unit 4 at -5.2e-7, and fp32 lands on the other side of that ReLU -- the gradient is not continuous there.  The unpartitioned
    engine and P = 2 both differ from the oracle by 1.03e-3 in proc1_node.W3 (TOL_GRAD is 2e-4), the difference is one outer product
    (singular values 5.7e-3, 1.4e-5, ...), and with that one mask entry on the other side the oracle is met to 6.8e-5.  Datapoint T - 2
    has no pre-activation that close: 3.1e-7 (L = 32) and 5.9e-7 (L = 128) for one partition and for P = 2 alike."""
    pr = problem(L, hl, scattered)
    e = engine_for(pr.cfg)
    pr.setup(e)
    pr.upload(e)
    got = dict(export={(t, n): e.datapoint_export(t, n) for t in range(T - 1) for n in (True, False)},
               step={t: e.step_datapoint(t, pr.mask) for t in (0, T - 2)}, renumbered=renumbered(e))
    e.close()
    nf, ef, tq = got["export"][(T - 2, True)]
    got["oracle"] = orc.step_grads(pr.ps, pr.cfg, nf, ef, pr.s, pr.r, tq, pr.mask)
    for v in list(got["export"].values()) + list(got["step"].values()) + [got["oracle"]]:
        for a in v:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return got


def check_references(pr, gs, loss, one, ref):
    """item 4: the one-partition step within the bound between two summation orders, the oracle within mgn_step's tolerances"""
    g1, l1 = one
    assert abs(loss - l1) <= TOL_LOSS * abs(l1), (loss, l1)
    assert rel_l2(gs, g1) <= TOL_ORDER
    ref_gs, ref_loss = ref
    assert abs(loss - ref_loss) <= TOL_LOSS * abs(ref_loss), (loss, ref_loss)
    print("worst tensor against the oracle:", check_grads(gs, ref_gs, pr.cfg, TOL_GRAD))


def code_of(call):
    with pytest.raises(MgnError) as ei:
        call()
    return ei.value.code


# ---- 1, 2, 4: exports, the step against step!, against one partition and the oracle --------------------------------------------------
@pytest.mark.parametrize("P,L,hl,scattered,stage_bytes", CASES)
def test_export_and_step_against_one_partition(monkeypatch, P, L, hl, scattered, stage_bytes):
    pr, one = problem(L, hl, scattered), single(L, hl, scattered)
    if scattered:
        assert one["renumbered"]
    if stage_bytes is not None:
        monkeypatch.setenv("MGN_TRAJ_STAGE_BYTES", str(stage_bytes))      # (a frame of the mesh is 10 560 bytes)
    with pr.group(P) as g:
        pr.setup(g)
        pr.upload(g)
        views = [g.rank_engine(k) for k in range(P)]
        assert all(v.n_halo > 0 and 0 < v.n_own < pr.N for v in views) and sum(v.n_own for v in views) == pr.N
        if scattered:
            assert all(renumbered(v) for v in views)
        # 1. export equals one partition, bit for bit: partition-independent noise, the chunked upload, the local-edge layout
        for t in (0, 1, T - 2):
            for normalised in (True, False):
                for name, a, b in zip(("nf", "ef", "target"), g.datapoint_export(t, normalised), one["export"][(t, normalised)]):
                    assert np.array_equal(a, b), (t, normalised, name)
        cur = g.datapoint_export(0, normalised=False)[0][:, :pr.cfg["O"]]
        assert np.array_equal(cur[~pr.noisy], pr.frames[0][~pr.noisy]) and np.all(cur[pr.noisy] != pr.frames[0][pr.noisy])
        # one rank alone: its own rows, the others untouched (no collective)
        own = views[P - 1].owned_nodes()
        eid = views[P - 1].local_edges()
        nf1, ef1, tq1 = views[P - 1].datapoint_export(1)
        nf_all, ef_all, tq_all = one["export"][(1, True)]
        other = np.setdiff1d(np.arange(pr.N), own)
        assert np.array_equal(nf1[own], nf_all[own]) and np.array_equal(tq1[own], tq_all[own]) and np.array_equal(ef1[eid], ef_all[eid])
        assert not nf1[other].any() and not tq1[other].any() and not ef1[np.setdiff1d(np.arange(pr.E), eid)].any()
        # 2. the step is step! on that datapoint: the same bits, with a 0-based and a 1-based mask
        for t in (0, T - 2):
            gs, loss = g.step_datapoint(t, pr.mask)
            assert np.isfinite(loss) and np.abs(gs).max() > 0
            gs_s, loss_s = g.step(*g.datapoint_export(t), pr.mask)
            assert loss == loss_s and same_bits(gs, gs_s), (t, loss, loss_s)
            gs_1, loss_1 = g.step_datapoint(t, pr.mask + 1, mask_index_base=1)
            assert loss_1 == loss and same_bits(gs_1, gs), t
            # 4. against one partition (both datapoints) and the oracle (datapoint T - 2: see single())
            g1, l1 = one["step"][t]
            assert abs(loss - l1) <= TOL_LOSS * abs(l1) and rel_l2(gs, g1) <= TOL_ORDER, (t, loss, l1)
            if t == T - 2:
                check_references(pr, gs, loss, one["step"][t], one["oracle"])


# ---- 3: every way of running P ranks agrees -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [2, 3])
def test_thread_ranks_over_the_host_transport_give_the_groups_bits(P):
    pr = problem()
    cid = mgn_amd.Engine.comm_unique_id("host")

    def run(e):
        out = [e.step_datapoint(0, pr.mask), e.step_datapoint(T - 2, pr.mask)]
        e.online_norms(max_acc=1e6)
        out.append(e.step_datapoint(1, pr.mask, accumulate=True))
        return [(np.array(gs), loss) for gs, loss in out], [e.norm_state(g) for g in range(3)]

    def body(k):
        e = engine_for(pr.cfg, rank=k, nranks=P, device=0)
        pr.setup(e)
        e.comm_init(cid, "host")
        pr.upload(e)
        got = run(e)
        e.comm_barrier()
        e.close()
        return got

    ranks = run_ranks(P, body)
    with pr.group(P) as g:
        pr.setup(g)
        pr.upload(g)
        steps, totals = run(g)
    for got, tot in ranks:                    # every rank: the group's bits
        for (gs, loss), (gs_g, loss_g) in zip(got, steps):
            assert loss == loss_g and same_bits(gs, gs_g)
        for a, b in zip(tot, totals):
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2:] == b[2:]
    assert steps[2][1] != steps[0][1]


# ---- 5: a rank that owns no mask entry and no noisy node ------------------------------------------------------------------------------
def test_a_rank_without_mask_entry_and_without_noisy_node():
    pr = problem()
    owner = mgn_amd.Engine.partition_nodes(pr.N, 2, mesh_pos=pr.pos)
    mask = np.nonzero(owner == 0)[0][::2].astype(np.int32)
    noisy = owner == 0
    assert mask.size > 0 and not np.any(owner[mask] == 1) and noisy.any() and not noisy[owner == 1].any()
    e = engine_for(pr.cfg)
    pr.setup(e)
    pr.upload(e, noise=False)
    e.set_noise(pr.stddev, noisy, seed=SEED)
    one = e.step_datapoint(1, mask)
    exp = e.datapoint_export(1)
    e.close()
    ref = orc.step_grads(pr.ps, pr.cfg, *exp[:2], pr.s, pr.r, exp[2], mask)
    with pr.group(2) as g:
        pr.setup(g)
        assert np.array_equal(g.rank_engine(1).node_owner(), owner)
        pr.upload(g, noise=False)
        g.set_noise(pr.stddev, noisy, seed=SEED)
        for a, b in zip(g.datapoint_export(1), exp):
            assert np.array_equal(a, b)
        gs, loss = g.step_datapoint(1, mask)
    check_references(pr, gs, loss, one, ref)


# ---- 6: online normalisers ------------------------------------------------------------------------------------------------------------
def maps_from_totals(tot, eps=1e-8):
    """the documented formula (include/mgn_hip.h): mean and std in double, rounded to float, std = max(std, eps); forward maps
    (scale = 1 / std, shift = -mean scale); for the output what read_maps returns: (1 / std, -mean / std)"""
    s, q, count, _ = tot
    c = max(count, 1.0)
    mean_d = s / c
    var = q / c - mean_d * mean_d
    mean, sd = mean_d.astype(F32), np.maximum(np.sqrt(np.maximum(var, 0.0)).astype(F32), F32(eps))
    scale = (F32(1.0) / sd).astype(F32)
    return scale, (-mean * scale).astype(F32), (-mean / sd).astype(F32)


@pytest.mark.parametrize("P", [2, 3])
def test_online_normalisers_across_ranks(P):
    pr = problem()
    N, E, O = pr.N, pr.E, pr.cfg["O"]
    want = [[0.0, 0.0, 0.0, 0.0] for _ in range(3)]      # float64 NumPy: sum, sum of squares, sum |x|, sum x^2
    rows = (N, E, N)
    with pr.group(P) as g:
        pr.setup(g)                                      # frozen maps first: the one-hot columns keep theirs
        pr.upload(g)
        views = [g.rank_engine(k) for k in range(P)]
        g.online_norms(max_acc=3, std_epsilon=1e-8)
        results, states = [], []
        for call, t in enumerate((0, 1, 2, 0)):
            capped = call == 3                           # max_accumulations reached: the totals stand still
            rnf, ref_, d = g.datapoint_export(t, normalised=False)
            if not capped:
                for gi, x in enumerate((rnf[:, :O], ref_, d)):
                    x = x.astype(np.float64)
                    want[gi] = [want[gi][0] + x.sum(0), want[gi][1] + (x * x).sum(0), want[gi][2] + np.abs(x).sum(0), want[gi][3] + (x * x).sum(0)]
            gs, loss = g.step_datapoint(t, pr.mask, accumulate=True)
            calls = min(call + 1, 3)
            tot = [g.norm_state(gi) for gi in range(3)]
            for gi in range(3):
                s_, q_, count, ncalls = tot[gi]
                for v in views:                          # identical bits on every rank
                    a = v.norm_state(gi)
                    assert np.array_equal(a[0], s_) and np.array_equal(a[1], q_) and a[2:] == (count, ncalls), (call, gi)
                assert count == calls * rows[gi] and ncalls == calls, (call, gi, count, ncalls)
                bound_s = calls * rows[gi] * 2.0 ** -52 * want[gi][2]       # a double summation of that many terms in any order
                bound_q = calls * rows[gi] * 2.0 ** -52 * want[gi][3]
                print(f"call {call} group {gi}: |sum - ref| / bound {np.abs(s_ - want[gi][0]) / bound_s}, squares {np.abs(q_ - want[gi][1]) / bound_q}")
                assert np.all(np.abs(s_ - want[gi][0]) <= bound_s) and np.all(np.abs(q_ - want[gi][1]) <= bound_q), (call, gi)
                if capped:
                    assert np.array_equal(s_, states[-1][gi][0]) and np.array_equal(q_, states[-1][gi][1])
            states.append(tot)
            # the step consumed what the export shows, and item 2 holds with online maps
            nf, ef, tq = g.datapoint_export(t)
            gs_s, loss_s = g.step(nf, ef, tq, pr.mask)
            assert loss_s == loss and same_bits(gs_s, gs), call
            gs_n, loss_n = g.step_datapoint(t, pr.mask)
            assert loss_n == loss and same_bits(gs_n, gs), call
            results.append((np.array(gs), loss))
            # the maps: the same on every rank (read_maps asserts that its probe rows, which all ranks wrote, agree) and the formula's
            g.set_noise()                                # (the probe rows carry no noise; pr.upload inside read_maps puts it back)
            (ns, nsh), (es, esh), (os_, osh) = read_maps(g, pr)
            fn, fe, fo = (maps_from_totals(tot[gi]) for gi in range(3))
            um = (ulps(ns, fn[0]), ulps(nsh, fn[1]), ulps(es, fe[0]), ulps(esh, fe[1]), ulps(os_, fo[0]), ulps(osh, fo[2]))
            print(f"call {call}: maps {um} ulp against the formula on the group's totals")
            assert max(um) <= 1.0, um
            assert np.array_equal(nf[:, O:], pr.onehot)
    # restored totals on a fresh group reproduce the next step's loss and gradients bit for bit: the state after two calls, then the third
    with pr.group(P) as g2:
        pr.setup(g2)
        pr.upload(g2)
        g2.online_norms(max_acc=3, std_epsilon=1e-8)
        for gi in range(3):
            g2.set_norm_state(gi, *states[1][gi])
        gs_r, loss_r = g2.step_datapoint(2, pr.mask, accumulate=True)
        assert loss_r == results[2][1] and same_bits(gs_r, results[2][0])
        for gi in range(3):
            a, b = g2.norm_state(gi), states[2][gi]
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


# ---- 7: lifecycle and refusals --------------------------------------------------------------------------------------------------------
def test_lifecycle_and_refusals():
    pr = problem()
    N = pr.N
    with pr.group(2) as g:
        pr.setup(g)
        assert code_of(lambda: g.step_datapoint(0, pr.mask)) == STATE          # no trajectory
        assert code_of(lambda: g.datapoint_export(0)) == STATE
        pr.upload(g)
        good = g.step_datapoint(0, pr.mask)
        good = (np.array(good[0]), good[1])

        def still_good():
            gs, loss = g.step_datapoint(0, pr.mask)
            assert loss == good[1] and same_bits(gs, good[0])

        # a second trajectory on the same graph, and the first one again
        g.set_trajectory(pr.frames[::-1].copy(), times=TIMES, node_type_onehot=pr.onehot, ef_raw=pr.ef_raw)
        assert g.step_datapoint(0, pr.mask)[1] != good[1]
        pr.upload(g, noise=False)                                             # (the noise settings hold on the same graph)
        still_good()
        # refusals of the group: before any collective, far sooner than the communicator's time-out; the next step gives the earlier bits
        bad = pr.mask.copy()
        bad[3] = N + 5
        loss = C.c_float()
        buf = np.zeros(g.param_count, F32)
        refused = [
            lambda: g.step_datapoint(T - 1, pr.mask),
            lambda: g.step_datapoint(-1, pr.mask),
            lambda: g._chk(g.lib.mgn_group_step_datapoint(g.g, 0, 0, i32(pr.mask), pr.mask.size, 0, f32(buf), buf.size - 1,
                                                          C.byref(loss))),
            lambda: g.step_datapoint(0, bad),
            lambda: g.step_datapoint(0, np.zeros(0, np.int32)),
            lambda: g.datapoint_export(T - 1),
            lambda: g.set_trajectory(pr.frames[:1], times=TIMES[:1], node_type_onehot=pr.onehot, ef_raw=pr.ef_raw),
        ]
        for i, call in enumerate(refused):
            t0 = time.monotonic()
            with pytest.raises(MgnError) as ei:
                call()
            took = time.monotonic() - t0
            assert ei.value.code == ARG and "rank" in str(ei.value), (i, str(ei.value))
            assert took < 10.0, (i, took)
            still_good()                                                      # (a refused upload leaves the trajectory alone, too)
        # a new graph drops the trajectory and the noise settings
        g.set_graph(pr.s, pr.r, N, mesh_pos=pr.pos)
        assert code_of(lambda: g.step_datapoint(0, pr.mask)) == STATE
        assert code_of(lambda: g.datapoint_export(0)) == STATE
        pr.upload(g)
        still_good()
    # two edge sets on a partitioned rank handle; a rank handle without a communicator names mgn_comm_init; a bf16 group
    c = pr.cfg
    two = mgn_amd.Engine(c["Fn"], c["Fe"], c["O"], 32, 2, c["mps"], rank=0, nranks=2, Fe2=4)
    two.set_graph(pr.s, pr.r, N, mesh_pos=pr.pos)
    bare = engine_for(c, rank=0, nranks=2, device=0)
    bare.set_graph(pr.s, pr.r, N, mesh_pos=pr.pos)
    kw = dict(times=TIMES, node_type_onehot=pr.onehot, ef_raw=pr.ef_raw)
    for e, want in ((two, UNSUPPORTED), (bare, STATE)):
        calls = (lambda: e.set_trajectory(pr.frames, **kw), lambda: e.set_noise(pr.stddev), lambda: e.online_norms(),
                 lambda: e.norm_state(0), lambda: e.step_datapoint(0, pr.mask), lambda: e.datapoint_export(0))
        for call in calls:
            with pytest.raises(MgnError) as ei:
                call()
            assert ei.value.code == want
            assert want != STATE or "mgn_comm_init" in str(ei.value)
        e.close()
    with GroupEngine(c["Fn"], c["Fe"], c["O"], 128, 2, c["mps"], devices=[0, 0], dtype="bf16") as half:
        half.set_graph(pr.s, pr.r, N, mesh_pos=pr.pos)
        for call in (lambda: half.set_trajectory(pr.frames, **kw), lambda: half.set_noise(pr.stddev), lambda: half.online_norms(),
                     lambda: half.norm_state(0), lambda: half.step_datapoint(0, pr.mask), lambda: half.datapoint_export(0)):
            assert code_of(call) == STATE
