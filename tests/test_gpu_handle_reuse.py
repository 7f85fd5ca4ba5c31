"""Every entry point on a handle that has held another mesh.

A production handle lives through thousands of trajectories (julia/MGNHip.jl calls mgn_set_graph whenever the graph key changes), so its
normal state is that its buffers hold the previous meshes' bytes: DevBuf::ensure keeps an allocation that still fits, and prepare_graph
lays a new offset table over the old training arena.  Each WALK below is one handle driven through a sequence of STOPS (set_graph, the
per-graph state of the entry point, the calls); it runs once, in a memo shared by the module, and the tests only compare what it
recorded.  At every stop:

  (a) the float64 oracle at the bounds of the module that owns the entry point (imported, not copied);
  (b) equal bits with a fresh handle given the same graph, parameters, inputs and switches;
  (c) the same call three times: equal bits (a small stop runs eagerly, captures its launch sequences, then replays them);
  (d) the regime that ran: train_regime counts and plan through test_gpu_training_regimes.expected_counts, last_kernels() family codes.

The poisoned variant of a walk runs, before it leaves a stop, the stop's fixed-step entry points once more with every floating-point
input NaN (never an index, a mask, a count or a row pointer; never an adaptive solve; never an accumulating normaliser).  The poison
result is asserted non-finite, so the pass reached the buffers; after it the arena, the kept activations, the gradient sets, the
partials, the ODE workspace and the encoded edges hold NaN, and the next stop must still give the bits of the fresh handle.  A stale
float that reaches a result then shows as NaN even where its reader multiplies it by a zero mask.

All walks run at the test CU count 8 (the regime switches sit at 64 tiles), renumbering off except where a stop names it.  Graphs and
inputs are those of test_gpu_training_regimes.inputs() and test_gpu_large_mesh_regimes.graph() where one fits; the new ones (the table
INPUTS of the host-only handle_reuse_inputs.py) went through tools/train_regime_inputs.py first, on the CPU (SEED_BUMP there records the
seeds it refused).  Mesh Q of walk 4 and mesh B of walk 5 are not in that table and were not screened; their errors are far inside
the bounds.

What NaN inputs reach.  The ReLU of the MLPs is a maximum with zero, which drops a NaN, so NaN features (nf, ef, x0, the one-hot
columns) stop at the first hidden layer: the poisoned forward of a step leaves finite activations behind, and mgn_forward / the resident
right-hand side answer NaN features with finite numbers (they are run in the poison pass, and not asserted on).  NaN targets, cotangents
(ybar, lam), states (x0 through x + dt f) and latents (latents_import, processor_steps) do travel: the loss, every gradient, nfbar / xbar,
the latents and the rollout's saves of every poison pass were non-finite.  Rows that no kernel ever writes -- the padding rows of the
tile-major arrays, the zero row of CARRY -- cannot be poisoned through an entry point; there check (b) is what bites, because a fresh
handle's allocations come back from the allocator with other handles' bytes in them (mutation 2 below).

The forward half.  So that the kept activations of the forward hold NaN as well, every poison pass ends with one call under NaN
PARAMETERS and finite inputs (poison_params_step; the parameters are put back at once): a NaN bias of an MLP's last Dense layer has no
ReLU behind it, so every kept Y, LayerNorm output, latent array V_k / E_k and aggregate, the decoder's output, mgn_forward's result and
the resident right-hand side's are NaN -- asserted: a NaN loss from finite inputs, no finite entry in forward's and the right-hand side's output.
Only the post-ReLU H1 / H2 cannot hold a NaN (they are all zero after that call).  A +Inf feature column does not get there either:
measured on three regimes (small A, 64 | 65 tiles, both streaming) it made the encoders' W1 gradients non-finite and nothing else, the
loss stayed finite -- the split of an infinite operand into pieces yields Inf - Inf = NaN ahead of layer 1's ReLU.

Measured on an MI355X (C = 8).  Every stop of every walk, plain and poisoned, was bit-equal to its fresh handle and to its own second and
third call, and plain and poisoned walks gave the same bits (the figures below are both).  The whole module (127 tests) takes 6.5 s, its
slowest test 0.8 s.  Error: the worst parameter tensor as in test_gpu_training_regimes.py; every loss was within 2e-7 of the oracle's.

walk             stop                     call  worst tensor           error     grad L2   worst nfbar / xbar row
step             both streaming           step  proc1_edge.b1          5.23e-07  2.32e-07  -
step             both streaming           vjp   enc_node.ln_scale      3.09e-06  1.28e-06  5.78e-07
step             64 | 65 tiles            step  proc1_node.W2          4.00e-05  4.76e-06  -
step             nodes streaming          step  enc_edge.b1            7.01e-07  3.40e-07  -
step             small A (both visits)    step  enc_node.W1            7.39e-07  3.97e-07  -
step             small A (both visits)    vjp   enc_edge.W1            8.93e-07  4.89e-07  4.01e-07
step             small A (both visits)    ode   enc_edge.W1            8.93e-07  4.89e-07  4.69e-07
step             65 | 65 tiles            step  enc_edge.ln_scale      7.42e-07  3.33e-07  -
step             small B                  step  enc_edge.W1            9.19e-07  5.16e-07  -
step             empty                    step  enc_node.W1            5.80e-07  3.89e-07  -
hidden_layers 3  hidden_layers 3          step  enc_edge.W3            7.92e-07  1.71e-07  -
hidden_layers 3  small hidden_layers 3    step  enc_edge.W1            8.32e-07  2.46e-07  -
ln_dims all      ln_dims all              step  proc0_node.W1          1.42e-06  6.89e-07  -
ln_dims all      small ln_dims all        step  proc0_node.ln_scale    1.17e-06  5.24e-07  -
second set       second set streaming     step  proc0_edge2.W1         8.45e-07  3.10e-07  -
second set       second set cooperative   step  proc0_edge2.b1         9.69e-07  2.92e-07  -
second set       empty second set         step  enc_edge.W2            2.42e-06  2.39e-07  -
renumbered       scattered grid           step  proc1_edge.W2          5.51e-07  2.40e-07  -
renumbered       small A                  step  enc_node.W1            7.39e-07  3.97e-07  -
group            mesh A (halo 33 + 33)    step  enc_node.W1            3.53e-05  -         -
group            mesh B (halo 20 + 20)    step  proc0_edge.W1          5.33e-07  -         -

inference, max |d| / max |ref| (bf16: relative L2)   forward   v         e         per row   right-hand side  rollout (rel. L2)
ring (17 | 17 tiles, both visits)   fp32  17 / 10    6.51e-07  3.53e-07  2.86e-07  5.48e-07  1.10e-06         4.16e-08
16-row (8 | 16 tiles)               fp32  15 / 8     8.51e-07  2.45e-07  2.13e-07  5.12e-07  6.00e-07         3.92e-08
ring (both visits)                  bf16  18 / 12    8.50e-03  5.03e-03  4.75e-03  -         8.53e-03         1.47e-04
16-row                              bf16  15 / 8     4.73e-03  3.17e-03  3.09e-03  -         4.79e-03         7.04e-05

datapoints and solver (L = 128, mps = 2): step_datapoint with accumulating normalisers, gradient relative L2 against the restatement:
mesh P 2.13e-07 / 2.27e-07 / 2.95e-07 (t = 0, 1, 2), mesh Q 2.00e-07 / 1.86e-07 / 2.23e-07, mesh P again 2.47e-07 / 1.91e-07 / 2.20e-07;
Euler solver_grad 2.44e-07 (P), 2.23e-07 (Q), 2.80e-07 (P again), losses within 4e-7; after every stop the totals were the restatement's
over all the stops so far, bit for bit.  The walk is P, Q, P: Q is the larger mesh (77 nodes against 48, more edges), so every buffer
sized by the mesh is allocated anew on arrival at Q and kept on the way back, and the second visit of P lays its arena, ODE workspace,
encoded edges, trajectory staging and adjoint workspace inside the bytes that Q's poison pass left.

Mutations (scratch builds, never committed; each changes only which in-bounds float is read or whether it is zeroed).  Beside this
module each ran the earlier modules named with it.  They were run when walk 4 had the two stops P, Q and before the NaN-parameter
pass was added: the counts are of the 123 tests of that state, and none of the four is a stale-memory mutation of the solver or
datapoint path.
 1. k_wgrad_h2's amax_zero no longer zeroes the rows past the end of a block (they repeat the block's first row): fails 31 tests here --
    23 of the 25 cases of test_training_stop_against_the_oracle, all 4 of the datapoint / solver and all 4 of the group oracle checks -- and
    14 tests of test_gpu_training_regimes.py.  It is no stale-memory mutation: the walked and the fresh handle agree.
 2. alloc_edge_set without its hipMemsetAsync (P, Q, Elat, AGG, CARRY keep their bytes): fails the 6 fp32 cases of
    test_inference_stop_equals_a_fresh_handle (the fresh handle, whose allocations hold other handles' bytes, computes something else), and 27
    tests of test_gpu_large_mesh_regimes.py and test_gpu_golden_and_partition.py; none of test_gpu_encdec_stages.py.
 3. the halo rows of SGr and gV not zeroed (mgn_train.cpp, the two memsets of the reverse pass): fails test_group_stop on mesh A, plain
    and poisoned, and test_gpu_partitioned_step.py::test_streaming_kernels_and_factored_first_layer; none of test_gpu_group.py.
 4. ef_pad_ok left set across prepare_graph: fails nothing here, nor in test_gpu_step_datapoint.py / test_gpu_step_datapoints.py: a new
    graph drops the trajectory (and the flag with it) before prepare_graph runs, so the line only matters when the arena is laid out
    again for the same graph (a changed test CU count), which no walk does.
"""
import numpy as np
import pytest
import torch  # noqa: F401  (before the engine's first HIP call)

import mgn_amd
import mgn_oracle as orc
from handle_reuse_inputs import INPUTS, VJP_INPUTS, inputs  # noqa: F401
import solver_adjoint_ref as sar
import test_gpu_bf16 as tb
import test_gpu_large_mesh_regimes as lm
import test_gpu_launch_state as ls
import test_gpu_partitioned_step as pp
import test_gpu_solver_train as st
import test_gpu_step_datapoint as sd
import test_gpu_training_regimes as tr
import test_gpu_training_step as ts
from mgn_amd import GroupEngine, synth
from mgn_amd import reference_api as ra
from util import TOL_15, TOL_ROLLOUT, last_kernels, rel_max, renumbered, set_renumber, small_mesh, train_regime

pytestmark = pytest.mark.gpu

C8 = 8
TILE = 32
rows_of = tr.rows_of

# ---- the new inputs live in handle_reuse_inputs.py (host only: tools/train_regime_inputs.py screens that table) --------------------
_refs = {}


def data(name):
    return tr.inputs(name) if name in tr.INPUTS else inputs(name)


def reference(name, vjp=False):
    """float64: (gradient, loss) of step!, or (gradient, nfbar) of the pullback for ybar -- computed once, shared, never written to"""
    if name in tr.INPUTS:
        return tr.reference(name, vjp)
    if (name, vjp) not in _refs:
        d = inputs(name)
        orc.LN_DIMS = "all" if d["lnall"] else "row"
        try:
            seed = (lambda out: d["ybar"].astype(np.float64)) if vjp else tr.loss_seed(d)
            out, gs, g_nf = orc.model_vjp(d["ps"], d["cfg"], d["nf"], d["ef"], d["s"], d["r"], seed, set2=d["set2"])
        finally:
            orc.LN_DIMS = "row"
        other = g_nf if vjp else float(orc.mse_reduce(d["target"].astype(np.float64), out)[d["mask"]].mean())
        gs.setflags(write=False)
        if vjp:
            other.setflags(write=False)
        _refs[(name, vjp)] = (gs, other)
    return _refs[(name, vjp)]


def nan_like(a):
    return np.full_like(a, np.nan)


def same(a, b):
    """equal bits of two results (arrays, floats, or tuples of them)"""
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32 if a.dtype == np.float32 else a.dtype),
                                                                        b.view(np.uint32 if b.dtype == np.float32 else b.dtype))


def finite(a):
    if isinstance(a, (tuple, list)):
        return all(finite(x) for x in a)
    return bool(np.isfinite(np.asarray(a)).all())


class Memo:
    """a walk runs once; an exception inside it is every one of its tests' failure"""

    def __init__(self):
        self.got = {}

    def __call__(self, key, fn):
        if key not in self.got:
            try:
                self.got[key] = (fn(), None)
            except BaseException as ex:       # noqa: BLE001
                self.got[key] = (None, ex)
        val, ex = self.got[key]
        if ex is not None:
            raise ex
        return val


@pytest.fixture(scope="module")
def memo():
    m = Memo()
    yield m
    m.got.clear()


# =================================================================================================================================
# walks 1 and 2: mgn_step, mgn_forward_vjp, mgn_ode_vjp
# =================================================================================================================================
def call_step(eng, d):
    gs, loss = eng.step(d["nf"], d["ef"], d["target"], d["mask"])
    return gs, np.float32(loss)


def call_vjp(eng, d):
    nfbar, gs, _ = eng.forward_vjp(d["nf"], d["ef"], d["ybar"])
    return gs, nfbar


def call_ode(eng, d):
    """mgn_ode_vjp under the handle's identity normalisers, no val_mask: x and the one-hot columns are the columns of nf, lam = ybar, so
    that the oracle's pullback of the model call for ybar is its reference (xbar = the first O columns of nfbar)"""
    xbar, gs, _ = eng.ode_vjp(d["nf"][:, :2], d["nf"][:, 2:], d["ef"], d["ybar"])
    return gs, xbar


def poison_step(eng, d):
    if d["set2"]:
        eng.set_edge_features(1, nan_like(d["set2"][0]))
    gs, loss = eng.step(nan_like(d["nf"]), nan_like(d["ef"]), nan_like(d["target"]), d["mask"])
    return gs, np.float32(loss)


def poison_params_step(eng, d):
    """the last pass of a stop: the step once more under NaN PARAMETERS, which are floating-point inputs too.  NaN features stop at the
    first ReLU (the docstring); a NaN bias of a last Dense layer, which no ReLU follows, does not: every kept Y, LayerNorm output, latent
    array and aggregate of the forward half of the arena is NaN after it (the post-ReLU H1 / H2 are all zero: a maximum with zero cannot
    give a NaN).  The parameters are put back before the walk goes on; the fresh handle never sees them."""
    eng.set_params(nan_like(d["ps"]))
    try:
        gs, loss = eng.step(d["nf"], d["ef"], d["target"], d["mask"])
    finally:
        eng.set_params(d["ps"])
    return gs, np.float32(loss)


def poison_vjp(eng, d):
    nfbar, gs, _ = eng.forward_vjp(d["nf"], d["ef"], nan_like(d["ybar"]))
    return gs, nfbar


def poison_ode(eng, d):
    xbar, gs, _ = eng.ode_vjp(d["nf"][:, :2], d["nf"][:, 2:], d["ef"], nan_like(d["ybar"]))
    return gs, xbar


CALLS = {"step": call_step, "vjp": call_vjp, "ode": call_ode}
POISON = {"step": poison_step, "vjp": poison_vjp, "ode": poison_ode}

SMALL_PLAN = dict(factored0=0, gsets=4, need_gt=1)       # cooperative, four gradient sets on the second stream, captured replay
S8 = tr.STREAM_PLAN

# walk -> [(stop, input, calls, node form, edge form(s), plan, the input of tr.INPUTS whose hidden_layers / mps the counts follow)]
WALKS = {
    "step": [
        ("both streaming", "both streaming", ("step", "vjp"), "s8", "s8", dict(S8, rpb_edge0=True, rpb_node=False, keep_steps=2), None),
        ("64 | 65 tiles", "64 | 65 tiles", ("step",), "coop", "s8", dict(factored0=1, gsets=1, need_gt=1), None),
        ("nodes streaming", "nodes streaming", ("step",), "s8", "coop", dict(factored0=0, gsets=1, need_gt=1, rpb_node=True, rpb_edge0=False), None),
        ("small A", "small A", ("step", "vjp", "ode"), "coop", "coop", SMALL_PLAN, "both streaming"),
        ("65 | 65 tiles", "65 | 65 tiles", ("step",), "s8", "s8", dict(S8, rpb_edge0=False, rpb_node=False), None),
        ("small A again", "small A", ("step", "vjp", "ode"), "coop", "coop", SMALL_PLAN, "both streaming"),
        ("small B", "small B", ("step",), "coop", "coop", SMALL_PLAN, "both streaming"),
        ("empty", "empty", ("step",), "coop", [], SMALL_PLAN, "both streaming"),          # (an edge set with E = 0 launches nothing)
    ],
    "hidden_layers 3": [
        ("hidden_layers 3", "hidden_layers 3", ("step",), "s8", "s8", dict(S8, rpb_edge0=True), None),
        ("small hidden_layers 3", "small hidden_layers 3", ("step",), "coop", "coop", SMALL_PLAN, "hidden_layers 3"),
    ],
    "ln_dims all": [
        ("ln_dims all", "ln_dims all", ("step",), "s8", "s8", dict(factored0=1, gsets=1, need_gt=1), None),
        ("small ln_dims all", "small ln_dims all", ("step",), "coop", "coop", SMALL_PLAN, "ln_dims all"),
    ],
    "second set": [
        ("second set streaming", "second set streaming", ("step",), "s8", ["s8", "s8"], dict(factored0=1, factored1=1, gsets=1, need_gt=0), None),
        ("second set cooperative", "second set cooperative", ("step",), "s8", ["s8", "coop"], dict(factored0=1, factored1=0, gsets=1, need_gt=1), None),
        ("empty second set", "empty second set", ("step",), "s8", ["s8"], dict(factored0=1, factored1=0, gsets=1, need_gt=0), "second set cooperative"),
    ],
    "renumbered": [      # renumbering on auto: the scattered grid is renumbered (g2l, ptmp, the mask remap), small A is not
        ("scattered grid", "scattered grid", ("step",), "coop", "s8", dict(factored0=1, gsets=1, need_gt=1), "both streaming"),
        ("small A", "small A", ("step",), "coop", "coop", SMALL_PLAN, "both streaming"),
    ],
}
VARIANTS = {"step": ("plain", "poisoned")}                # the other walks run poisoned only
RENUMBER = {"renumbered": (True, False)}                  # mgn_debug_renumbered per stop


def new_engine(d):
    cfg = d["cfg"]
    eng = mgn_amd.Engine(9, 3, 2, 128, cfg["hidden_layers"], cfg["mps"], Fe2=cfg.get("Fe2"), ln_dims="all" if d["lnall"] else 0)
    eng.set_params(d["ps"])
    return eng


def enter(eng, d):
    eng.set_graph(d["s"], d["r"], d["N"])
    if d["set2"]:
        eng.set_edge_set(1, d["set2"][1], d["set2"][2])
        eng.set_edge_features(1, d["set2"][0])


def thrice(eng, d, call):
    res = []
    for i in range(3):
        train_regime(None, reset=True)
        res.append(CALLS[call](eng, d))
        if i == 0:
            regime = train_regime(eng, reset=True)
    return dict(res=res, regime=regime)


class TrainSwitches(tr.Switches):
    def __init__(self, walk):
        super().__init__(C8)
        self.walk = walk

    def __enter__(self):
        super().__enter__()
        if self.walk in RENUMBER:
            set_renumber(1)               # (tr.Switches puts the old value back)
        return self


def run_walk(walk, poisoned):
    """one handle through the stops of the walk: per stop {call: {res: three results, regime of the first}, poison: {call: result}}"""
    recs, eng = [], None
    with TrainSwitches(walk):
        try:
            for stop, name, calls, *_ in WALKS[walk]:
                d = data(name)
                if eng is None:
                    eng = new_engine(d)
                enter(eng, d)
                rec = {"renumbered": renumbered(eng)}
                for c in calls:
                    rec[c] = thrice(eng, d, c)
                if poisoned:
                    rec["poison"] = {c: POISON[c](eng, d) for c in calls}
                    rec["poison_params"] = poison_params_step(eng, d)
                recs.append(rec)
        finally:
            if eng is not None:
                eng.close()
    return recs


def run_fresh(walk):
    """every stop of the walk on a handle of its own"""
    recs = []
    with TrainSwitches(walk):
        for stop, name, calls, *_ in WALKS[walk]:
            d = data(name)
            eng = new_engine(d)
            try:
                enter(eng, d)
                recs.append({c: CALLS[c](eng, d) for c in calls})
            finally:
                eng.close()
    return recs


def walked(memo, walk, variant):
    return memo((walk, variant), lambda: run_fresh(walk) if variant == "fresh" else run_walk(walk, variant == "poisoned"))


TRAIN_STOPS = [pytest.param(w, v, i, id=f"{w}-{v}-{i}:{WALKS[w][i][0]}")
               for w in WALKS for v in VARIANTS.get(w, ("poisoned",)) for i in range(len(WALKS[w]))]


def check_oracle(name, call, got):
    """the bounds of test_gpu_training_regimes.check (step, forward_vjp) and of test_ode_vjp_matches_oracle_and_ode_step (ode_vjp)"""
    d = data(name)
    gs, other = got
    ref, ref2 = reference(name, call != "step")
    assert finite(got)
    errs = tr.tensor_errors(gs, ref, d["cfg"])
    worst = max(errs, key=errs.get)
    l2 = float(np.linalg.norm(gs - ref) / np.linalg.norm(ref))
    line = f"{name} {call}: worst tensor {worst} {errs[worst]:.2e}, gradient L2 {l2:.2e}"
    if call == "step":
        print(f"{line}, loss {float(other)!r} against {ref2!r}")
        assert abs(float(other) - ref2) <= tr.TOL_LOSS * abs(ref2), (other, ref2)
        assert l2 <= tr.TOL_L2 and errs[worst] <= tr.TOL_GRAD, (worst, errs[worst], l2)
    elif call == "vjp":
        rows = tr.nf_row_errors(other, ref2)
        nl2 = float(np.linalg.norm(other - ref2) / np.linalg.norm(ref2))
        print(f"{line}, nfbar worst row {rows.max():.2e}, rows over {tr.TOL_GRAD}: {(rows > tr.TOL_GRAD).sum()}, L2 {nl2:.2e}")
        assert (rows > tr.TOL_GRAD).sum() <= tr.MAX_BAD_ROWS and nl2 <= tr.TOL_NF_L2, ((rows > tr.TOL_GRAD).sum(), rows.max(), nl2)
        assert l2 <= tr.TOL_L2 and errs[worst] <= tr.TOL_GRAD, (worst, errs[worst], l2)
    else:
        rx = ref2[:, :2]
        rows = np.abs(other - rx).max(1) / np.abs(rx).max()
        xl2 = float(np.linalg.norm(other - rx) / np.linalg.norm(rx))
        print(f"{line}, xbar worst row {rows.max():.2e}, L2 {xl2:.2e}")
        assert np.quantile(rows, 0.98) <= ts.TOL_GRAD, np.quantile(rows, 0.98)
        assert xl2 <= 5e-3 and l2 <= 5e-3, (xl2, l2)
        ts.check_grads(gs, ref, d["cfg"], tol=2e-2)


@pytest.mark.parametrize("walk,variant,i", TRAIN_STOPS)
def test_training_stop_against_the_oracle(memo, walk, variant, i):
    """(a) every entry point of the stop, its first call"""
    stop, name, calls, *_ = WALKS[walk][i]
    rec = walked(memo, walk, variant)[i]
    for c in calls:
        check_oracle(name, c, rec[c]["res"][0])


@pytest.mark.parametrize("walk,variant,i", TRAIN_STOPS)
def test_training_stop_equals_a_fresh_handle(memo, walk, variant, i):
    """(b) the bits of a handle that has held nothing else; (c) three calls, equal bits"""
    stop, name, calls, *_ = WALKS[walk][i]
    rec, fresh = walked(memo, walk, variant)[i], walked(memo, walk, "fresh")[i]
    for c in calls:
        a, b, c3 = rec[c]["res"]
        assert same(a, b) and same(a, c3), f"{stop}: {c} is not repeatable on the walked handle"
        assert finite(fresh[c])
        assert same(a, fresh[c]), f"{stop}: {c} differs from the fresh handle (stale memory reaches the result)"


@pytest.mark.parametrize("walk,variant,i", TRAIN_STOPS)
def test_training_stop_ran_its_regime(memo, walk, variant, i):
    """(d) launches by form and the plan of the arena, of the stop's first call (later calls of a small stop replay captured launches,
    and the forward sequence is shared between the entry points); forward_vjp as well where nothing is captured"""
    stop, name, calls, node, edge, plan, like = WALKS[walk][i]
    rec = walked(memo, walk, variant)[i]
    want = tr.expected_counts(like or name, node, edge)
    for c in calls[:1] + tuple(c for c in calls[1:] if node == "s8"):
        regime = rec[c]["regime"]
        for k in ("fwd", "bwd", "lin2"):
            assert regime[k] == want[k], (stop, c, k, regime[k], want[k])
        for k, v in plan.items():
            if k.startswith("rpb"):
                assert (regime[k] > 192) == v, (stop, c, k, regime[k])
            else:
                assert regime[k] == v, (stop, c, k, regime[k], v)
    if walk in RENUMBER:
        assert rec["renumbered"] == RENUMBER[walk][i], (stop, rec["renumbered"])


@pytest.mark.parametrize("walk,i", [pytest.param(w, i, id=f"{w}-{i}:{WALKS[w][i][0]}") for w in WALKS for i in range(len(WALKS[w]))])
def test_training_poison_reached_the_buffers(memo, walk, i):
    """the poison pass of the stop gave nothing finite: its NaN went through the arena to the loss, the gradient and the input gradient"""
    stop, name, calls, *_ = WALKS[walk][i]
    rec = walked(memo, walk, "poisoned")[i]
    for c in calls:
        gs, other = rec["poison"][c]
        assert not finite(gs) and not finite(other), (stop, c)
    gs, loss = rec["poison_params"]
    assert not finite(gs) and not finite(loss), stop     # finite inputs: a NaN loss is a NaN output of the forward (a W1 gradient behind a closed ReLU is 0)


# =================================================================================================================================
# walk 3: inference and the resident right-hand side
# =================================================================================================================================
DT = 0.01
# The "cylinder-sized mesh on the 16-row cooperative kernels" of the plan: at the test CU count 8 those kernels take at most 8 node tiles
# and 16 edge tiles, so the stop is the largest graph that still runs them (256 nodes, 511 edges), not a mesh of the cylinder's size -- the
# regime is the one meant (family codes 15 / 8, asserted), the size is what C = 8 scales it down to.
N_C16, E_C16 = rows_of(8, 32), rows_of(16, 31)
# (stop, (N, E), family codes of the last processor step: fp32, bf16 -- DESIGN.md section 2)
INFER_STOPS = [("ring", (ls.N_PROC, ls.E_PROC), (17, 10), (18, 12)),
               ("16-row", (N_C16, E_C16), (15, 8), (15, 8)),
               ("ring again", (ls.N_PROC, ls.E_PROC), (17, 10), (18, 12))]
INFER_CALLS = ("forward", "proc", "rhs", "rollout")
_infer = {}


def infer_data(N, E):
    """inputs of the four entry points on lm.graph(N, E) and their float64 results (identity normalisers: the right-hand side is the
    model on [x ; one-hot])"""
    if (N, E) not in _infer:
        s, r, v, e, rv, re = lm.graph(N, E)
        rng = np.random.default_rng(N * 7 + E)
        d = dict(s=s, r=r, N=N, E=E, v=v, e=e)
        d["nf"] = rng.standard_normal((N, 9)).astype(np.float32)
        d["ef"] = rng.standard_normal((E, 3)).astype(np.float32)
        d["x"] = rng.standard_normal((N, 2)).astype(np.float32)
        d["onehot"] = np.eye(7, dtype=np.float32)[rng.integers(0, 7, N)]
        ps = lm.params()

        def rhs(x):
            return orc.forward(ps, lm.CFG, np.concatenate([x, d["onehot"]], 1), d["ef"], s, r)

        xs = [d["x"].astype(np.float64)]
        for _ in range(5):
            xs.append(xs[-1] + float(np.float32(DT)) * rhs(xs[-1]))
        d["ref"] = dict(forward=orc.forward(ps, lm.CFG, d["nf"], d["ef"], s, r), proc=(rv, re), rhs=rhs(d["x"].astype(np.float64)),
                        rollout=np.stack(xs))
        for a in d.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _infer[(N, E)] = d
    return _infer[(N, E)]


def infer_calls(eng, d, nan=False):
    """the four entry points once; nan: with every floating-point input NaN"""
    p = nan_like if nan else (lambda a: a)
    out = {"forward": eng.forward(p(d["nf"]), p(d["ef"])), "proc": eng.processor_steps(p(d["v"]), p(d["e"]), lm.NSTEPS)}
    out["fam"] = last_kernels()
    eng.set_static(p(d["onehot"]), p(d["ef"]))
    out["rhs"] = eng.ode_step(p(d["x"]))
    out["rollout"] = eng.rollout("Euler", p(d["x"]), p(d["onehot"]), p(d["ef"]), 0.0, 5 * DT, DT, 6, dt=DT)[0]
    return out


def infer_stop(eng, d, poisoned):
    eng.set_graph(d["s"], d["r"], d["N"])
    runs = [infer_calls(eng, d)]
    eng.set_static(d["onehot"], d["ef"])
    for _ in range(3):                                            # the resident right-hand side: eager, captured, replayed
        runs.append(dict(rhs=eng.ode_step(d["x"])))
    for _ in range(2):                                            # every entry point a second and a third time
        runs.append(infer_calls(eng, d))
    rec = dict(runs=runs)
    eng.fwd_upload(d["nf"], d["ef"])
    eng.fwd_encode()
    rec["encode"] = eng.latents_export() + (eng.latents_checksum(),)
    if poisoned:
        rec["poison"] = infer_calls(eng, d, nan=True)
        eng.set_params(nan_like(lm.params()))                     # NaN parameters reach what NaN features cannot (poison_params_step)
        try:
            rec["poison"]["forward_params"] = eng.forward(d["nf"], d["ef"])
            eng.set_static(d["onehot"], d["ef"])
            rec["poison"]["rhs_params"] = eng.ode_step(d["x"])
        finally:
            eng.set_params(lm.params())
        eng.latents_import(nan_like(d["v"]), nan_like(d["e"]))
    return rec


def run_infer(dtype, variant):
    recs = []
    with lm.Switches(C8):
        eng = None
        try:
            for stop, (N, E), *_ in INFER_STOPS:
                d = infer_data(N, E)
                if eng is None or variant == "fresh":
                    if eng is not None:
                        eng.close()
                    eng = mgn_amd.Engine(9, 3, 2, 128, 2, lm.NSTEPS, dtype=dtype)
                    eng.set_params(lm.params())
                recs.append(infer_stop(eng, d, variant == "poisoned"))
        finally:
            if eng is not None:
                eng.close()
    return recs


def inferred(memo, dtype, variant):
    return memo(("infer", dtype, variant), lambda: run_infer(dtype, variant))


INFER_PARAMS = [pytest.param(dt, v, i, id=f"{dt}-{v}-{i}:{INFER_STOPS[i][0]}")
                for dt, vs in (("f32", ("plain", "poisoned")), ("bf16", ("poisoned",))) for v in vs for i in range(len(INFER_STOPS))]


def rel_l2(a, ref):
    return tb.rel_l2(np.asarray(a, np.float64), np.asarray(ref, np.float64))


@pytest.mark.parametrize("dtype,variant,i", INFER_PARAMS)
def test_inference_stop_against_the_oracle(memo, dtype, variant, i):
    """(a) forward, processor_steps, the resident right-hand side and an Euler rollout: fp32 at TOL_15 / ROW_TOL / TOL_ROLLOUT, bf16 at its
    band; (d) the family codes of the last processor step; and the padding rows of the tile-major arrays read as zero after
    fwd_encode: the device's sums over whole tiles are the sums of the exported rows"""
    stop, (N, E), fam32, fam16 = INFER_STOPS[i]
    d = infer_data(N, E)
    rec = inferred(memo, dtype, variant)[i]
    got, ref = rec["runs"][0], d["ref"]
    assert all(finite(got[c]) for c in INFER_CALLS)
    (v1, e1), (rv, re) = got["proc"], ref["proc"]
    if dtype == "f32":
        err = dict(forward=rel_max(got["forward"], ref["forward"]), v=rel_max(v1, rv), e=rel_max(e1, re), rhs=rel_max(got["rhs"], ref["rhs"]),
                   rows=max(lm.row_err(v1, rv), lm.row_err(e1, re)), rollout=rel_l2(got["rollout"], ref["rollout"]))
        print(f"{stop} {dtype} {variant}: families {got['fam']}, {err}")
        assert got["fam"] == fam32, got["fam"]
        assert max(err["forward"], err["v"], err["e"], err["rhs"]) <= TOL_15, err
        assert err["rows"] <= lm.ROW_TOL and err["rollout"] <= TOL_ROLLOUT, err
    else:
        err = dict(forward=rel_l2(got["forward"], ref["forward"]), v=rel_l2(v1, rv), e=rel_l2(e1, re), rhs=rel_l2(got["rhs"], ref["rhs"]),
                   rollout=rel_l2(got["rollout"], ref["rollout"]))
        print(f"{stop} {dtype} {variant}: families {got['fam']}, {err}")
        assert got["fam"] == fam16, got["fam"]
        assert max(err.values()) <= tb.TOL_BF16, err
    v, e, chk = rec["encode"]
    v64, e64 = v.astype(np.float64), e.astype(np.float64)
    for what, have, want in (("sum_v", chk["sum_v"], v64.sum()), ("sumsq_v", chk["sumsq_v"], (v64 * v64).sum()),
                             ("sum_e", chk["sum_e"], e64.sum()), ("sumsq_e", chk["sumsq_e"], (e64 * e64).sum())):
        assert np.isclose(have, want, rtol=1e-9, atol=0.0), (stop, what, have, want)


@pytest.mark.parametrize("dtype,variant,i", INFER_PARAMS)
def test_inference_stop_equals_a_fresh_handle(memo, dtype, variant, i):
    """(b) and (c): every call of the stop, its repeats, the encoded latents and their checksum"""
    stop = INFER_STOPS[i][0]
    rec, fresh = inferred(memo, dtype, variant)[i], inferred(memo, dtype, "fresh")[i]
    first = rec["runs"][0]
    for k, run in enumerate(rec["runs"][1:] + fresh["runs"]):
        where = f"call {k + 2} on the walked handle" if k + 1 < len(rec["runs"]) else "the fresh handle"
        for c in INFER_CALLS:
            assert c not in run or same(first[c], run[c]), f"{stop}: {c} differs from {where}"
    assert same(rec["encode"][:2], fresh["encode"][:2]) and rec["encode"][2] == fresh["encode"][2], f"{stop}: fwd_encode"
    if variant == "poisoned":
        # The poison pass reached the outputs, so it went through the buffers: no finite latent row, no finite row of the rollout's
        # last save.  (forward and the right-hand side take NaN features as well, but the first ReLU of the encoders is a maximum
        # with zero, which drops a NaN: their results are finite and only say that the input buffers were written.)
        assert not np.isfinite(rec["poison"]["forward_params"]).any() and not np.isfinite(rec["poison"]["rhs_params"]).any(), stop
        v, e = rec["poison"]["proc"]
        assert not np.isfinite(v).any(1).any() and not np.isfinite(e).any(1).any(), stop
        assert not np.isfinite(rec["poison"]["rollout"][-1]).any(1).any(), stop


# =================================================================================================================================
# walk 4: derivative training on a resident trajectory with online normalisers, and solver-based training
# =================================================================================================================================
SG = (0.0, 0.03, 0.01, 0.01, 4)                     # t0, t1, dt, saves_dt, n_saves of the Euler solve: the T = 4 frames are its saves
LOSS_SCALE = np.array([1.0, 2.0], np.float32)
_dp = {}


DP_STOPS = (0, 1, 0)                                # P, Q, P again: Q is the larger mesh, so the buffers sized by the mesh are re-allocated on
#                                                     arrival at Q and KEPT on the way back -- the second visit of P lies inside Q's poisoned bytes
DP_NAMES = ("mesh P", "mesh Q", "mesh P again")


def dp_problem(i):
    """mesh P: test_gpu_step_datapoint's own problem (48 nodes, two node tiles); mesh Q: another N and E (77 nodes, three node tiles,
    more edges), filled in the same way.  (Neither went through tools/train_regime_inputs.py, which screens the INPUTS table only: P is the
    owning module's problem as it stands.  Should a gradient bound fail here on the walked AND the fresh handle alike, look for a ReLU
    kink in the input before a defect in the engine.)"""
    if i not in _dp:
        p = sd.Problem()
        if i == 1:
            p.pos, p.s, p.r = small_mesh(11, 7, seed=4)
            N, E = p.N, p.E = p.pos.shape[0], p.s.size
            rng = np.random.default_rng(6)
            p.frames = (rng.standard_normal((sd.T, N, sd.O)) * np.array([1.2, 0.4]) + np.array([1.5, -0.3])).astype(np.float32)
            p.types = rng.integers(0, sd.NTYPES, N)
            p.onehot = ra.one_hot(p.types, sd.NTYPES)
            p.ef_raw = (rng.standard_normal((E, sd.FE)) * np.array([0.3, 0.1, 0.2]) + np.array([0.1, 0.0, 0.2])).astype(np.float32)
            p.mask = np.sort(rng.choice(N, int(0.6 * N), replace=False)).astype(np.int32)
            p.noisy = (p.types != 1)
            p.data = {"velocity": p.frames[:-1], "target|velocity": p.frames[1:]}
        p.vm = (p.types != 1).astype(np.float32)
        _dp[i] = p
    return _dp[i]


def dp_model():
    cfg = sd.cfg_of(128)
    return cfg, sd.params_of(cfg)


def solver_call(eng, p, nan=False):
    q = nan_like if nan else (lambda a: a)
    gs, loss = eng.solver_grad(q(p.frames[0]), q(p.onehot), q(p.ef_raw), q(p.frames), *SG, val_mask=p.vm, loss_scale=LOSS_SCALE)
    return gs, np.float32(loss)


def dp_stop(eng, k, state, poisoned, restore=None):
    """state: the host restatement that lives through the walk (the three NormaliserOnline mirrors and the float64 totals), or None on a
    fresh handle, which is given the walked handle's totals of the stop before (restore) instead"""
    p = dp_problem(DP_STOPS[k])
    cfg, ps = dp_model()
    eng.set_graph(p.s, p.r, p.N)
    p.upload(eng)                                                 # set_trajectory again: a new graph drops it
    eng.set_noise(p.stddev, p.noisy, seed=11 + k)                 # and the noise
    if restore is not None:
        for g in range(3):
            eng.set_norm_state(g, *restore[g])
    rec = dict(acc=[], acc_ref=[])
    if state is not None:
        raw = [eng.datapoint_export(t, normalised=False) for t in range(sd.T - 1)]
        noisy = {"velocity": np.stack([x[0][:, :sd.O] for x in raw]), "target|velocity": p.frames[1:]}     # (the target's next state carries no noise)
    for t in range(sd.T - 1):
        if state is not None:
            raws = (np.ascontiguousarray(raw[t][0][:, :sd.O]), raw[t][1], raw[t][2])
            for g in range(3):
                s_, q_ = eng.feature_stats(raws[g])
                state["tot"][g][0] += s_
                state["tot"][g][1] += q_
                state["tot"][g][2] += raws[g].shape[0]
                state["tot"][g][3] += 1
        gs, loss = eng.step_datapoint(t, p.mask, accumulate=True)
        rec["acc"].append((gs, np.float32(loss)))
        if state is not None:
            mnf, mef, mtq = p.mirror(t, {"dt": float(sd.DT)}, state["mgn"], noisy)
            rec["acc_ref"].append(p.oracle(ps, cfg, mnf, mef, mtq))
    rec["totals"] = [eng.norm_state(g) for g in range(3)]
    rec["dp"] = []
    for _ in range(3):                                            # the maps as they stand: eager, captured, replayed
        gs, loss = eng.step_datapoint(sd.T - 2, p.mask)
        rec["dp"].append((gs, np.float32(loss)))
    rec["sg"] = [solver_call(eng, p) for _ in range(3)]
    if state is not None:
        rec["want_totals"] = [(a.copy(), b.copy(), c, k) for a, b, c, k in state["tot"]]
        on_n, on_e, on_o = state["mgn"].n_norm["velocity"].frozen(), state["mgn"].e_norm.frozen(), state["mgn"].o_norm["velocity"].frozen()
        P = dict(cfg=cfg, ps=ps, onehot=p.onehot, ef_raw=p.ef_raw, s=p.s, r=p.r, vm=p.vm, t_norm=orc.NormMinMax(0.0, 1.0),
                 n_norm=orc.NormMeanStd(on_n.mean, on_n.std), e_norm=orc.NormMeanStd(on_e.mean, on_e.std),
                 o_norm=orc.NormMeanStd(on_o.mean, on_o.std))
        o_rhs, o_vjp, _ = st.oracle_fns(P)
        rec["sg_ref"] = sar.euler_adjoint(o_rhs, o_vjp, p.frames[0], p.frames, *SG, val_mask=p.vm, loss_scale=LOSS_SCALE)[:2]
    if poisoned:                                                  # (step_datapoint stays out: its normalisers accumulate)
        rec["poison"] = dict(sg=solver_call(eng, p, nan=True),
                             rollout=eng.rollout("Euler", nan_like(p.frames[0]), nan_like(p.onehot), nan_like(p.ef_raw), 0.0, 0.03, 0.01, 4, dt=0.01)[0],
                             step=eng.step(np.full((p.N, sd.FN), np.nan, np.float32), nan_like(p.ef_raw), nan_like(p.frames[0]), p.mask))
        eng.set_params(nan_like(ps))                              # NaN parameters, finite inputs: the forward half of the arena (poison_params_step)
        try:
            rec["poison"]["step_params"] = eng.step(np.zeros((p.N, sd.FN), np.float32), p.ef_raw, p.frames[0], p.mask)
        finally:
            eng.set_params(ps)
    return rec


def dp_engine():
    cfg, ps = dp_model()
    eng = sd.engine_of(cfg)
    eng.set_params(ps)
    eng.set_norms(**dp_problem(0).norms())                        # the one-hot columns keep these maps
    eng.online_norms(max_acc=1e6, std_epsilon=1e-8)
    return eng


def run_dp(variant, walked_totals=None):
    recs = []
    with tr.Switches(C8):
        if variant == "fresh":
            for k in range(len(DP_STOPS)):
                eng = dp_engine()
                try:
                    recs.append(dp_stop(eng, k, None, False, restore=walked_totals[k - 1] if k else None))
                finally:
                    eng.close()
            return recs
        frozen = dp_problem(0).frozen
        state = dict(mgn=sd.Mgn({"velocity": ra.NormaliserOnline(sd.O), "node_type": frozen.n_norm["node_type"]},
                                ra.NormaliserOnline(sd.FE), {"velocity": ra.NormaliserOnline(sd.O)}),
                     tot=[[np.zeros(d), np.zeros(d), 0.0, 0.0] for d in (sd.O, sd.FE, sd.O)])
        eng = dp_engine()
        try:
            for k in range(len(DP_STOPS)):
                recs.append(dp_stop(eng, k, state, variant == "poisoned"))
        finally:
            eng.close()
    return recs


def dp_walked(memo, variant):
    if variant == "fresh":
        totals = [rec["totals"] for rec in dp_walked(memo, "plain")]
        return memo(("dp", "fresh"), lambda: run_dp("fresh", totals))
    return memo(("dp", variant), lambda: run_dp(variant))


DP_PARAMS = [pytest.param(v, i, id=f"{v}-{i}:{DP_NAMES[i]}") for v in ("plain", "poisoned") for i in range(len(DP_STOPS))]


@pytest.mark.parametrize("variant,i", DP_PARAMS)
def test_datapoint_and_solver_stop_against_the_oracle(memo, variant, i):
    """(a) step_datapoint with accumulating online normalisers against the host restatement of test_gpu_step_datapoint.py fed the noisy
    raw rows (its TOL_LOSS / TOL_GRAD), the Euler solver_grad under the maps as they then stand against tests/solver_adjoint_ref.py
    (the bounds of test_gpu_solver_train.py: loss 1e-4, gradient 5e-3 relative L2); and the contract that the online totals outlive
    graphs: after every stop they are the restatement's, accumulated over all the stops so far"""
    rec = dp_walked(memo, variant)[i]
    for t, ((gs, loss), (ref, ref_loss)) in enumerate(zip(rec["acc"], rec["acc_ref"])):
        gerr = float(np.linalg.norm(gs - ref) / np.linalg.norm(ref))
        print(f"{DP_NAMES[i]} {variant} t={t}: loss {loss} vs {ref_loss}, gradient rel L2 {gerr:.2e}")
        assert np.isfinite(gs).all()
        assert abs(loss - ref_loss) <= sd.TOL_LOSS * abs(ref_loss) and gerr <= sd.TOL_GRAD, (t, loss, ref_loss, gerr)
    (gs, loss), (ref, ref_loss) = rec["sg"][0], rec["sg_ref"]
    print(f"{DP_NAMES[i]} {variant} solver_grad: loss {loss} vs {ref_loss}, gradient rel L2 {st.rel_l2(gs, ref):.2e}")
    assert np.isfinite(gs).all()
    assert abs(loss - ref_loss) <= 1e-4 * abs(ref_loss) and st.rel_l2(gs, ref) <= 5e-3, (loss, ref_loss, st.rel_l2(gs, ref))
    rows = [(dp_problem(j).N, dp_problem(j).E, dp_problem(j).N) for j in DP_STOPS[:i + 1]]
    for g, ((s_, q_, count, calls), (ws, wq, wcount, wcalls)) in enumerate(zip(rec["totals"], rec["want_totals"])):
        assert np.array_equal(s_, ws) and np.array_equal(q_, wq), (g, s_, ws)
        assert count == wcount == (sd.T - 1) * sum(r[g] for r in rows) and calls == wcalls == (sd.T - 1) * (i + 1), (g, count, calls)


@pytest.mark.parametrize("variant,i", DP_PARAMS)
def test_datapoint_and_solver_stop_equals_a_fresh_handle(memo, variant, i):
    """(b) a fresh handle that is given the totals the walked one had on arrival; (c) repeats"""
    rec, fresh = dp_walked(memo, variant)[i], dp_walked(memo, "fresh")[i]
    for t in range(sd.T - 1):
        assert same(rec["acc"][t], fresh["acc"][t]), f"accumulating step_datapoint({t})"
    for what in ("dp", "sg"):
        a, b, c = rec[what]
        assert same(a, b) and same(a, c), f"{what} is not repeatable on the walked handle"
        assert finite(fresh[what][0]) and same(a, fresh[what][0]), f"{what} differs from the fresh handle"
    for a, b in zip(rec["totals"], fresh["totals"]):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2:] == b[2:]
    if variant == "poisoned":
        p = rec["poison"]
        assert not finite(p["sg"][0]) and not finite(p["sg"][1]) and not finite(p["step"][0]) and not finite(p["step_params"][0]) and not finite(p["step_params"][1]) and not np.isfinite(p["rollout"][-1]).any(1).any()


# =================================================================================================================================
# walk 5: a group of two partitions on one GPU
# =================================================================================================================================
_group = {}


def group_data(i):
    """mesh A: the 40 x 33 grid of test_gpu_partitioned_step.py; mesh B: a 24 x 20 grid -- smaller, and cut elsewhere.  (Mesh B's inputs
    did not go through tools/train_regime_inputs.py, which screens the INPUTS table only: should its bound fail on the walked and the
    fresh group alike, look for a ReLU kink in the input first.)"""
    if i not in _group:
        cfg, pos, s, r, ps, nf, ef, target, mask, ref, ref_loss = pp.grid_case()
        if i == 1:
            pos, cells = synth.grid_mesh(24, 20, 4)
            s, r = synth.cells_to_edges(cells)
            nf, ef, target, mask = pp.problem(cfg, pos, s, r, seed=5)
            ref, ref_loss = orc.step_grads(ps, cfg, nf, ef, s, r, target, mask)
        _group[i] = dict(cfg=cfg, pos=pos, s=s, r=r, N=pos.shape[0], ps=ps, nf=nf, ef=ef, target=target, mask=mask, ref=ref, ref_loss=ref_loss)
    return _group[i]


def run_group(variant):
    recs, g = [], None
    with tr.Switches(C8):
        try:
            for i in range(2):
                d = group_data(i)
                cfg = d["cfg"]
                if g is None or variant == "fresh":
                    if g is not None:
                        g.close()
                    g = GroupEngine(cfg["Fn"], cfg["Fe"], cfg["O"], cfg["L"], cfg["hidden_layers"], cfg["mps"], devices=[0, 0])
                    g.set_params(d["ps"])
                g.set_graph(d["s"], d["r"], d["N"], mesh_pos=d["pos"])
                rec = dict(halo=[g.rank_engine(k).n_halo for k in range(2)], own=[g.rank_engine(k).n_own for k in range(2)], res=[])
                for _ in range(3):
                    gs, loss = g.step(d["nf"], d["ef"], d["target"], d["mask"])
                    rec["res"].append((np.array(gs), np.float32(loss)))
                if variant == "poisoned":
                    gs, loss = g.step(nan_like(d["nf"]), nan_like(d["ef"]), nan_like(d["target"]), d["mask"])
                    rec["poison"] = (np.array(gs), np.float32(loss))
                    g.set_params(nan_like(d["ps"]))               # and under NaN parameters, finite inputs (poison_params_step)
                    try:
                        gs, loss = g.step(d["nf"], d["ef"], d["target"], d["mask"])
                    finally:
                        g.set_params(d["ps"])
                    rec["poison_params"] = (np.array(gs), np.float32(loss))
                recs.append(rec)
        finally:
            if g is not None:
                g.close()
    return recs


@pytest.mark.parametrize("variant,i", [pytest.param(v, i, id=f"{v}-{i}:mesh {'AB'[i]}") for v in ("plain", "poisoned") for i in range(2)])
def test_group_stop(memo, variant, i):
    """GroupEngine.step at P = 2 (hx_send / hx_recv, the accumulate CSR, the halo rows of SGr / gV over stale bytes): the oracle at the
    bounds of test_gpu_partitioned_step.py, the bits of a fresh group, three equal calls"""
    d = group_data(i)
    rec = memo(("group", variant), lambda: run_group(variant))[i]
    fresh = memo(("group", "fresh"), lambda: run_group("fresh"))[i]
    assert all(n > 0 for n in rec["halo"]) and sum(rec["own"]) == d["N"], rec
    gs, loss = rec["res"][0]
    assert np.isfinite(gs).all()
    assert abs(loss - d["ref_loss"]) <= pp.TOL_LOSS * abs(d["ref_loss"]), (loss, d["ref_loss"])
    print(f"mesh {'AB'[i]} {variant}: halo {rec['halo']}, worst tensor {pp.check_grads(gs, d['ref'], d['cfg'])}")
    assert same(rec["res"][0], rec["res"][1]) and same(rec["res"][0], rec["res"][2]), "step is not repeatable on the walked group"
    assert same(rec["res"][0], fresh["res"][0]), "step differs from the fresh group"
    if variant == "poisoned":
        assert not finite(rec["poison"][0]) and not finite(rec["poison"][1])
        assert not finite(rec["poison_params"][0]) and not finite(rec["poison_params"][1])


def test_no_switch_is_left():
    from util import set_num_cus, set_train_f16
    assert set_num_cus(0) == 0 and set_train_f16(1) == 1 and set_renumber(1) == 1
