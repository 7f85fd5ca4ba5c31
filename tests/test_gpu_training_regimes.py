"""Every large-mesh regime of the training step (mgn_step, mgn_forward_vjp) on oracle-sized graphs.

The size rules of the training launches -- cooperative kernels up to 8 tiles per CU, eight-tile streaming blocks above that (and with them
the aggregation fused into the edge forward, the LayerNorm sums inside the backward kernel, the factored first edge layer, one set of
gradient buffers, GT / GXH shrunk to placeholders), weight-gradient blocks of more than 192 rows above 4 blocks per CU -- are written for
256 CUs: 2048 tiles, 65 536 rows, where the float64 oracle takes minutes and a whole-gradient bound hides a wrong row.  With the test CU
count (mgn_debug_num_cus, C = 8) the same rules switch at 64 tiles and 6144 rows, and orc.step_grads / orc.model_vjp check every tensor
and every row of nfbar.  Each case asserts what ran (mgn_debug_train_regime: launches per form, and the plan of the arena; DESIGN.md
section 2), so a moved threshold fails here instead of silently testing another kernel.

Graphs are the ragged ones of test_gpu_large_mesh_regimes.py (synth.random_graph with seed 7 plus hubs): a receiver run over a dozen edge
tiles, a second hub mid-graph, node 0 sending and receiving 40 edges, the last N // 8 nodes receiving nothing, last tiles of 1, 31 or 32
rows.  Parameters: seed 1234, jitter 0.1; inputs: rng(N + E + E2), bumped per input where needed (SEED_BUMP).

Input choice.  A pre-activation within fp32 rounding of a ReLU kink makes float32 itself differ from float64 by percents in a few rows,
so every (graph, cfg) below went through tools/train_regime_inputs.py first, on the CPU: orc.model_vjp in float32 against float64, and
float64 against itself with every parameter moved by one fp32 rounding (8 draws) -- a kernel sums in another order than NumPy, so one
float32 run is one sample of the rounding.  An input is kept only where neither shows an nfbar row over 2e-5 or a tensor over 1e-5
(ln_dims = ALL: float32 takes the whole-array statistics in float32 and is off by up to 5e-5 in the LayerNorm parameters on every seed;
there the perturbation test alone carries the kink criterion); otherwise its seed is bumped (SEED_BUMP).  That criterion reads the
oracle only.  The bounds are the project's: loss 1e-5, whole-gradient relative L2 1e-3, per tensor TOL_GRAD = 2e-4, nfbar rows TOL_GRAD on
all but at most 8 rows (a condition, not a measurement: fewer than the 16 rows of a half tile, so a lost tile, half tile or wave cannot
hide under it) and 5e-3 relative L2; the default fp16-piece kernels may be at most twice as far from the oracle as the fp32-MFMA forms on
the same inputs, plus 2e-6 (the float32 oracle's own level).

Measured on an MI355X.  Error: the worst parameter tensor, max |d| / max(max |ref| of the tensor, 1e-3 max |ref| of the gradient); nfbar row:
the worst row, max |d| over the row / max |ref| of nfbar (no row was over TOL_GRAD in any case); the last column is the same pair on the
fp32-MFMA forms where the 2 x rule compares them ("C = 8 fp32" rows: case 10 itself).  Every loss was within 8e-8 of the oracle's.

input                    CU count     call  worst tensor           error     grad L2   nfbar row  fp32-MFMA forms: tensor / row
both streaming           C = 8        step  proc1_edge.b1          5.23e-07  2.32e-07  -          2.23e-07 / -
both streaming           no override  step  proc1_edge.W1          6.63e-07  2.44e-07  -
65 | 65 tiles            C = 8        step  enc_edge.ln_scale      7.42e-07  3.33e-07  -
64 | 65 tiles            C = 8        step  proc1_node.W2          4.00e-05  4.76e-06  -
nodes streaming          C = 8        step  enc_edge.b1            7.01e-07  3.40e-07  -          5.95e-07 / -
nodes streaming          no override  step  enc_edge.b1            5.20e-07  2.93e-07  -
65.1 | 71.32             C = 8        step  enc_edge.ln_scale      5.98e-07  2.74e-07  -
65.32 | 71.1             C = 8        step  proc1_node.b1          8.02e-07  3.27e-07  -
71.1 | 72.32             C = 8        step  proc0_node.b1          5.88e-07  3.00e-07  -
71.32 | 72.1             C = 8        step  proc1_node.b1          7.46e-07  3.52e-07  -
72.1 | 65.32             C = 8        step  proc0_edge.ln_scale    6.11e-07  2.99e-07  -
72.32 | 65.1             C = 8        step  proc1_node.W1          6.19e-07  3.34e-07  -
three steps              C = 8        step  proc2_edge.W1          3.83e-07  2.01e-07  -
hidden_layers 3          C = 8        step  enc_edge.W3            7.92e-07  1.71e-07  -
hidden_layers 1          C = 8        step  enc_node.W1            2.54e-07  1.38e-07  -
second set cooperative   C = 8        step  proc0_edge2.b1         9.69e-07  2.92e-07  -
second set streaming     C = 8        step  proc0_edge2.W1         8.45e-07  3.10e-07  -
ln_dims all              C = 8        step  proc0_node.W1          1.42e-06  6.89e-07  -
both streaming           C = 8        vjp   enc_node.ln_scale      3.09e-06  1.28e-06  5.78e-07   1.09e-06 / 1.00e-06
nodes streaming          C = 8        vjp   proc0_node.b1          3.57e-06  1.39e-06  4.62e-07   1.38e-06 / 6.28e-07
both streaming           C = 8 fp32   step  enc_node.W3            2.23e-07  9.97e-08  -
nodes streaming          C = 8 fp32   step  enc_edge.W1            5.95e-07  1.20e-07  -
both streaming           C = 8 fp32   vjp   proc1_edge.ln_scale    1.09e-06  7.23e-07  1.00e-06
nodes streaming          C = 8 fp32   vjp   proc1_edge.W2          1.38e-06  5.24e-07  6.28e-07

Mutations (scratch builds): the last partial block dropped from the LayerNorm sums of the node launches of k_mlp_bwd<.., 8, ..> fails 11
tests here and none of the earlier streaming tests; the forced need_gt = false (edge sets left out of the rule) fails the 5 tests with a
cooperative edge set beside streaming nodes (MGN_E_STATE from the guard in bwd_unit) and none of the earlier ones; the k_seg_fixup carry
skipped across eight-tile blocks fails 15 tests here, and both earlier streaming tests as well.  Rounding wgrad_rows_per_block down
instead of up does not fail: every user reads the same function and rows per block stay a multiple of 16, so the launch only gets more
blocks than the cap.
"""
import numpy as np
import pytest
import torch  # noqa: F401  (before the engine's first HIP call)

import mgn_amd
import mgn_oracle as orc
from mgn_amd import synth
from util import set_num_cus, set_renumber, set_train_f16, train_regime

pytestmark = pytest.mark.gpu

TILE = 32
C8 = 8
TOL_LOSS = 1e-5      # as tests/test_gpu_training_step.py
TOL_GRAD = 2e-4
TOL_L2 = 1e-3        # whole gradient, relative L2
TOL_NF_L2 = 5e-3     # whole nfbar, relative L2
MAX_BAD_ROWS = 8
FLOOR_2X = 2e-6


def rows_of(T, tail):
    """rows of T tiles whose last one holds `tail` rows (1, 31 or 32)"""
    return (T - 1) * TILE + tail


# name -> (N, E, hidden_layers, mps, ln_dims ALL, rows of the second edge set)
INPUTS = {
    "both streaming": (rows_of(100, 1), rows_of(300, 31), 2, 2, False, 0),                    # case 1
    "65 | 65 tiles": (rows_of(65, 31), rows_of(65, 1), 2, 2, False, 0),                       # case 2
    "64 | 65 tiles": (rows_of(64, 32), rows_of(65, 1), 2, 2, False, 0),
    "nodes streaming": (rows_of(200, 32), rows_of(40, 31), 2, 2, False, 0),                   # case 3
    "65.1 | 71.32": (rows_of(65, 1), rows_of(71, 32), 2, 2, False, 0),                        # case 4
    "65.32 | 71.1": (rows_of(65, 32), rows_of(71, 1), 2, 2, False, 0),
    "71.1 | 72.32": (rows_of(71, 1), rows_of(72, 32), 2, 2, False, 0),
    "71.32 | 72.1": (rows_of(71, 32), rows_of(72, 1), 2, 2, False, 0),
    "72.1 | 65.32": (rows_of(72, 1), rows_of(65, 32), 2, 2, False, 0),
    "72.32 | 65.1": (rows_of(72, 32), rows_of(65, 1), 2, 2, False, 0),
    "three steps": (rows_of(100, 1), rows_of(300, 31), 2, 3, False, 0),                       # case 5
    "hidden_layers 3": (rows_of(100, 1), rows_of(300, 31), 3, 2, False, 0),                   # case 6
    "hidden_layers 1": (rows_of(100, 1), rows_of(300, 31), 1, 2, False, 0),
    "second set cooperative": (rows_of(100, 1), rows_of(300, 31), 2, 2, False, rows_of(20, 1)),   # case 7
    "second set streaming": (rows_of(100, 1), rows_of(300, 31), 2, 2, False, rows_of(70, 31)),
    "ln_dims all": (rows_of(100, 1), rows_of(300, 31), 2, 2, True, 0),                        # case 8
}
REMAINDERS = ("65.1 | 71.32", "65.32 | 71.1", "71.1 | 72.32", "71.32 | 72.1", "72.1 | 65.32", "72.32 | 65.1")                   # case 4
VJP_INPUTS = ("both streaming", "nodes streaming")                                            # case 9

# inputs: rng(N + E + E2 + 100003 k); k != 0 where tools/train_regime_inputs.py found k = 0 unfit (float32 alone crosses a ReLU kink there)
SEED_BUMP = {"65 | 65 tiles": 1, "nodes streaming": 1, "71.32 | 72.1": 2, "72.32 | 65.1": 1, "three steps": 13, "hidden_layers 3": 5,
             "second set cooperative": 2, "second set streaming": 4}

_graphs, _inputs, _refs, _fp32 = {}, {}, {}, {}


def graph(N, E):
    """the ragged graph of the inference regime test: built once, shared, never written to"""
    if (N, E) not in _graphs:
        s, r = synth.random_graph(N, E, 7)                        # the last N // 8 nodes receive nothing
        h1, h2 = min(12 * TILE + 5, E // 3), min(70, E // 8)
        r[:h1] = 3                                                # a run over a dozen edge tiles
        r[E // 2: E // 2 + h2] = N // 2                           # a second hub in the middle
        s[E // 4: E // 4 + 40] = 0                                # node 0 sends and receives
        r[3 * (E // 4): 3 * (E // 4) + 40] = 0
        first_empty = N - N // 8
        assert r.max() < first_empty and (first_empty + TILE - 1) // TILE * TILE + TILE <= N   # a whole node tile and the last node: no incoming edge
        s.setflags(write=False)
        r.setflags(write=False)
        _graphs[(N, E)] = (s, r)
    return _graphs[(N, E)]


def inputs(name):
    """cfg, parameters, graph and data of an input of INPUTS (host only: tools/train_regime_inputs.py reads them too)"""
    if name not in _inputs:
        N, E, hl, mps, lnall, E2 = INPUTS[name]
        cfg = dict(Fn=9, Fe=3, O=2, L=128, hidden_layers=hl, mps=mps)
        if E2:
            cfg["Fe2"] = 4
        ps = orc.init_params(9, 3, 2, 128, hl, mps, 1234, 0.1, Fe2=cfg.get("Fe2"))
        s, r = graph(N, E)
        rng = np.random.default_rng(N + E + E2 + 100003 * SEED_BUMP.get(name, 0))
        d = dict(cfg=cfg, ps=ps, N=N, E=E, s=s, r=r, lnall=lnall, set2=None)
        d["nf"] = rng.standard_normal((N, 9)).astype(np.float32)
        d["ef"] = rng.standard_normal((E, 3)).astype(np.float32)
        d["target"] = rng.standard_normal((N, 2)).astype(np.float32)
        d["mask"] = np.sort(rng.choice(N, int(0.6 * N), replace=False)).astype(np.int32)
        d["ybar"] = rng.standard_normal((N, 2)).astype(np.float32)
        if E2:
            s2, r2 = synth.random_graph(N, E2, 8)
            r2[:70] = 5                                           # a run over three tiles of the second set
            d["set2"] = (rng.standard_normal((E2, 4)).astype(np.float32), s2, r2)
        for v in d.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _inputs[name] = d
    return _inputs[name]


def loss_seed(d, dtype=np.float64):
    """the cotangent of the model's output under step!'s loss (orc.step_grads)"""
    target, mask = d["target"].astype(dtype), d["mask"]

    def seed(out):
        g = np.zeros_like(out)
        np.add.at(g, mask, 2.0 * (out[mask] - target[mask]) / mask.size)
        return g
    return seed


def oracle(name, vjp=False, dtype=np.float64):
    """float64: (gradient, loss) of step!, or (gradient, nfbar) of the pullback for ybar -- computed once, shared, never written to"""
    d = inputs(name)
    orc.LN_DIMS = "all" if d["lnall"] else "row"
    try:
        seed = (lambda out: d["ybar"].astype(dtype)) if vjp else loss_seed(d, dtype)
        out, gs, g_nf = orc.model_vjp(d["ps"], d["cfg"], d["nf"], d["ef"], d["s"], d["r"], seed, dtype=dtype, set2=d["set2"])
    finally:
        orc.LN_DIMS = "row"
    if vjp:
        return gs, g_nf
    return gs, float(orc.mse_reduce(d["target"].astype(np.float64), out)[d["mask"]].mean())


def reference(name, vjp=False):
    if (name, vjp) not in _refs:
        a, b = oracle(name, vjp)
        a.setflags(write=False)
        if vjp:
            b.setflags(write=False)
        _refs[(name, vjp)] = (a, b)
    return _refs[(name, vjp)]


def tensor_errors(gs, ref, cfg):
    """max |d| / max(max |ref| of the tensor, 1e-3 max |ref| of the gradient) per parameter tensor (check_grads of test_gpu_training_step.py)"""
    off, errs = 0, {}
    for bname, tensors in orc.model_layout(cfg["Fn"], cfg["Fe"], cfg["O"], cfg["L"], cfg["hidden_layers"], cfg["mps"], cfg.get("Fe2")):
        for tname, shape in tensors:
            n = int(np.prod(shape))
            a, b = gs[off:off + n], ref[off:off + n]
            errs[f"{bname}.{tname}"] = float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-3 * np.abs(ref).max()))
            off += n
    assert off == ref.size == gs.size
    return errs


def nf_row_errors(nfbar, ref):
    return np.abs(nfbar.astype(np.float64) - ref).max(1) / np.abs(ref).max()


class Switches:
    """the test CU count and the arithmetic form of a case; everything restored on exit"""

    def __init__(self, cus, f16=1):
        self.cus, self.f16, self.old = cus, f16, []

    def __enter__(self):
        rc = set_num_cus(self.cus)                                # (before any other switch: nothing to restore if this is refused)
        if rc != 0:
            if rc > 0:
                set_num_cus(rc)                                   # an override leaked from elsewhere: put it back and say so
            raise AssertionError(f"mgn_debug_num_cus({self.cus}) returned {rc}: an override was active, or this one was refused")
        self.old.append((set_num_cus, 0))
        self.old.append((set_renumber, set_renumber(0)))          # the graph's raggedness is built by node number
        self.old.append((set_train_f16, set_train_f16(self.f16)))
        return self

    def __exit__(self, *exc):
        for fn, val in reversed(self.old):
            fn(val)
        return False


def run(name, cus, f16=1, vjp=False):
    """mgn_step (or mgn_forward_vjp) twice on an input under the switches: (gradient, loss or nfbar, regime of the first call)"""
    d = inputs(name)
    cfg = d["cfg"]
    with Switches(cus, f16):
        eng = mgn_amd.Engine(9, 3, 2, 128, cfg["hidden_layers"], cfg["mps"], Fe2=cfg.get("Fe2"), ln_dims="all" if d["lnall"] else 0)
        try:
            eng.set_params(d["ps"])
            eng.set_graph(d["s"], d["r"], d["N"])
            if d["set2"]:
                eng.set_edge_set(1, d["set2"][1], d["set2"][2])
                eng.set_edge_features(1, d["set2"][0])
            res = []
            for i in range(2):
                train_regime(None, reset=True)
                if vjp:
                    nfbar, gs, _ = eng.forward_vjp(d["nf"], d["ef"], d["ybar"])
                    res.append((gs, nfbar))
                else:
                    res.append(eng.step(d["nf"], d["ef"], d["target"], d["mask"]))
                if i == 0:
                    regime = train_regime(eng, reset=True)
        finally:
            eng.close()
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(np.asarray(res[0][1]), np.asarray(res[1][1]))   # two calls: equal bits
    return res[0][0], res[0][1], regime


def expected_counts(name, node, edge, keep=None, f16=1):
    """Launches of one call by form.  node / edge: "coop" or "s8" per side (edge: one per set); every MLP is one launch unit (two from
    hidden_layers 3), node side: encoder, decoder, one per step; edge side: encoder, one per step; a recomputed step runs its forwards
    again; the factored first layer of a streaming edge set adds a launch_lin2 over the node tiles per forward and backward."""
    N, E, hl, mps, lnall, E2 = INPUTS[name]
    nb = 2 if hl >= 3 else 1
    rec = mps - (mps if keep is None else keep)
    edge = edge if isinstance(edge, (list, tuple)) else [edge]
    fwd, bwd, lin2 = {"coop": 0, "s4": 0, "s8": 0}, {"coop": 0, "s4": 0, "s8": 0}, {"coop": 0, "s4": 0, "s8": 0}
    fwd[node] += nb * (2 + mps + rec)
    bwd[node] += nb * (2 + mps)
    for form in edge:
        fwd[form] += nb * (1 + mps + rec)
        bwd[form] += nb * (1 + mps)
        if form != "coop":
            lin2["s8" if node == "s8" else "s4"] += 2 * mps + rec
    out = {}
    for k, c in (("fwd", fwd), ("bwd", bwd), ("lin2", lin2)):
        out[k] = (c["coop"], c["s4"], c["s8"], sum(c.values()) if f16 else 0)
    return out


def fp32_errors(name, cus, vjp):
    """the same input on the fp32-MFMA forms (mgn_debug_train_f16(0)) at the same CU count: (worst tensor error, worst nfbar row error)"""
    if (name, cus, vjp) not in _fp32:
        gs, other, regime = run(name, cus, f16=0, vjp=vjp)
        assert regime["fwd"][3] == regime["bwd"][3] == regime["lin2"][3] == 0, regime      # no launch on fp16 pieces
        ref, ref2 = reference(name, vjp)
        _fp32[(name, cus, vjp)] = (max(tensor_errors(gs, ref, inputs(name)["cfg"]).values()),
                                   float(nf_row_errors(other, ref2).max()) if vjp else 0.0, regime)
    return _fp32[(name, cus, vjp)]


def check(name, cus, node, edge, plan, keep=None, f16=1, vjp=False, two_x=False):
    """A case: counts and plan, then loss, whole-gradient L2, per tensor; for a pullback every row of nfbar.  Returns the gradient and
    the loss (or nfbar)."""
    d = inputs(name)
    gs, other, regime = run(name, cus, f16, vjp)
    want = expected_counts(name, node, edge, keep, f16)
    ref, ref2 = reference(name, vjp)
    errs = tensor_errors(gs, ref, d["cfg"])
    worst = max(errs, key=errs.get)
    l2 = float(np.linalg.norm(gs - ref) / np.linalg.norm(ref))
    print(f"{name} C={cus} f16={f16} vjp={vjp}: {regime}; worst tensor {worst} {errs[worst]:.2e}, gradient L2 {l2:.2e}", end="")
    for k in ("fwd", "bwd", "lin2"):
        assert regime[k] == want[k], (k, regime[k], want[k])
    for k, v in plan.items():
        if k.startswith("rpb"):
            assert (regime[k] > 192) == v, (k, regime[k])
        else:
            assert regime[k] == v, (k, regime[k], v)
    assert np.isfinite(gs).all()
    if vjp:
        rows = nf_row_errors(other, ref2)
        nl2 = float(np.linalg.norm(other - ref2) / np.linalg.norm(ref2))
        print(f", nfbar worst row {rows.max():.2e}, rows over {TOL_GRAD}: {(rows > TOL_GRAD).sum()}, L2 {nl2:.2e}")
        assert (rows > TOL_GRAD).sum() <= MAX_BAD_ROWS, ((rows > TOL_GRAD).sum(), rows.max())
        assert nl2 <= TOL_NF_L2, nl2
    else:
        print(f", loss {other!r} against {ref2!r}")
        assert abs(other - ref2) <= TOL_LOSS * abs(ref2), (other, ref2)
    assert l2 <= TOL_L2, l2
    assert errs[worst] <= TOL_GRAD, (worst, errs[worst])
    if two_x and f16:
        t32, r32, _ = fp32_errors(name, cus, vjp)
        print(f"    fp32-MFMA forms: worst tensor {t32:.2e}, worst nfbar row {r32:.2e}")
        assert errs[worst] <= 2.0 * t32 + FLOOR_2X, (errs[worst], t32)
        if vjp:
            assert float(rows.max()) <= 2.0 * r32 + FLOOR_2X, (float(rows.max()), r32)
    return gs, other


STREAM_PLAN = dict(factored0=1, gsets=1, need_gt=0)


@pytest.mark.parametrize("cus", [C8, 0], ids=["C=8", "no override"])
def test_both_sides_streaming(cus):
    """case 1: 100 node tiles, 300 edge tiles.  C = 8: every launch on eight-tile blocks, factored first layer, one gradient-buffer set,
    GT / GXH placeholders, 304 rows per edge weight-gradient block.  No override: the same input on the cooperative kernels, second-stream
    weight gradients (four sets), GT / GXH rows -- the same bounds, so the two regimes are compared on identical inputs."""
    if cus:
        check("both streaming", cus, "s8", "s8", dict(STREAM_PLAN, rpb_edge0=True, rpb_node=False, keep_steps=2), two_x=True)
    else:
        check("both streaming", 0, "coop", "coop", dict(factored0=0, gsets=4, need_gt=1, rpb_edge0=False, rpb_node=False))


def test_just_across_the_threshold():
    """case 2: 65 tiles on both sides are streaming throughout; 64 node tiles are the last cooperative size, beside 65 streaming edge tiles
    (the factored first layer's launch_lin2 then runs four-tile blocks over the nodes, and the cooperative node units need GT / GXH rows)"""
    check("65 | 65 tiles", C8, "s8", "s8", dict(STREAM_PLAN, rpb_edge0=False, rpb_node=False))
    check("64 | 65 tiles", C8, "coop", "s8", dict(factored0=1, gsets=1, need_gt=1))


@pytest.mark.parametrize("cus", [C8, 0], ids=["C=8", "no override"])
def test_nodes_streaming_edges_cooperative(cus):
    """case 3: 200 node tiles, 40 edge tiles: the un-factored edge MLP hands GXs / GXr to the segmented sums and writes GT / GXH rows, the
    streaming node units take their LayerNorm sums inside the backward kernel; 208 rows per node weight-gradient block"""
    if cus:
        check("nodes streaming", cus, "s8", "coop", dict(factored0=0, gsets=1, need_gt=1, rpb_node=True, rpb_edge0=False), two_x=True)
    else:
        check("nodes streaming", 0, "coop", "coop", dict(factored0=0, gsets=4, need_gt=1, rpb_node=False))


@pytest.mark.parametrize("name", REMAINDERS)
def test_eight_tile_block_remainders(name):
    """case 4: 65, 71 and 72 tiles (one, seven and no tile in the last eight-tile block) on the node and on the edge side, each with a last
    tile of 1 and of 32 rows"""
    N, E = INPUTS[name][:2]
    assert {(N + 31) // 32, (E + 31) // 32} <= {65, 71, 72}
    check(name, C8, "s8", "s8", STREAM_PLAN)


def test_recomputed_steps(monkeypatch):
    """case 5: three processor steps with three, one and none of them stored (MGN_TRAIN_KEEP_STEPS is read at every graph setup): equal
    bits, and the first against the oracle"""
    res = []
    for keep in (3, 1, 0):
        monkeypatch.setenv("MGN_TRAIN_KEEP_STEPS", str(keep))
        plan = dict(STREAM_PLAN, keep_steps=keep)
        if keep == 3:
            res.append(check("three steps", C8, "s8", "s8", plan, keep=keep))
        else:
            gs, loss, regime = run("three steps", C8)
            want = expected_counts("three steps", "s8", "s8", keep)
            assert all(regime[k] == want[k] for k in want) and all(regime[k] == v for k, v in plan.items()), (regime, want)
            res.append((gs, loss))
    for gs, loss in res[1:]:
        assert loss == res[0][1] and np.array_equal(gs, res[0][0])


@pytest.mark.parametrize("hl", [3, 1])
def test_hidden_layers_3_and_1(hl):
    """case 6: hidden_layers 3 runs two launch units per MLP (the second hands its input gradient to the first through GXB), 1 a single
    unit with an identity slot"""
    check(f"hidden_layers {hl}", C8, "s8", "s8", dict(STREAM_PLAN, rpb_edge0=True))


def test_two_edge_sets_with_streaming_nodes():
    """case 7: the node MLP of three inputs on eight-tile blocks.  A second set of 20 tiles stays cooperative and un-factored beside the
    factored first set (Pn / Qn / SGs / SGr and GXs / GXr all in use, GT / GXH rows for the cooperative units); one of 70 tiles streams"""
    check("second set cooperative", C8, "s8", ["s8", "coop"], dict(factored0=1, factored1=0, gsets=1, need_gt=1))
    check("second set streaming", C8, "s8", ["s8", "s8"], dict(factored0=1, factored1=1, gsets=1, need_gt=0))


def test_whole_array_layernorm():
    """case 8: ln_dims = MGN_LN_ALL at case 1's sizes: the streaming kernels stop at Y, per-tile statistics, GT / GXH rows"""
    check("ln_dims all", C8, "s8", "s8", dict(factored0=1, gsets=1, need_gt=1))


@pytest.mark.parametrize("name", VJP_INPUTS)
def test_forward_vjp_every_row(name):
    """case 9: mgn_forward_vjp at cases 1 and 3; every row of nfbar"""
    if name == "both streaming":
        check(name, C8, "s8", "s8", STREAM_PLAN, vjp=True, two_x=True)
    else:
        check(name, C8, "s8", "coop", dict(factored0=0, gsets=1, need_gt=1), vjp=True, two_x=True)


@pytest.mark.parametrize("name", VJP_INPUTS)
@pytest.mark.parametrize("vjp", [False, True], ids=["step", "vjp"])
def test_fp32_mfma_streaming_forms(name, vjp):
    """case 10: cases 1 and 3 with mgn_debug_train_f16(0): the same launches, none on fp16 pieces, the same bounds"""
    edge = "s8" if name == "both streaming" else "coop"
    plan = STREAM_PLAN if name == "both streaming" else dict(factored0=0, gsets=1, need_gt=1)
    check(name, C8, "s8", edge, plan, f16=0, vjp=vjp)


def test_no_switch_is_left_and_default_dispatch_is_unchanged():
    """After this module no override or switch is set, and with none the 2 300-edge-tile graph of
    test_step_streaming_kernels_on_a_graph_with_hubs_and_isolated_nodes still runs its 282 node tiles on the cooperative kernels (four
    forward and four backward launches), its edge side on eight-tile blocks (three each) and the factored first layer's launch_lin2 on
    four-tile blocks over the nodes: the literals 2048 / 2048 / 1024 stand."""
    assert set_num_cus(0) == 0 and set_train_f16(1) == 1 and set_renumber(1) == 1
    rng = np.random.default_rng(31)
    N, E = 9000, 73600
    deg = rng.integers(0, 31, N)
    deg[rng.choice(N, N // 10, replace=False)] = 0
    deg[17] = 300
    deg[N - 1] = 0
    r = np.repeat(np.arange(N), deg)
    r = np.concatenate([r, rng.integers(0, N, max(0, E - r.size))])[:E].astype(np.int32)
    s = rng.integers(0, N, E).astype(np.int32)
    assert (E + 31) // 32 == 2300
    nf = rng.standard_normal((N, 9)).astype(np.float32)
    ef = rng.standard_normal((E, 3)).astype(np.float32)
    target = rng.standard_normal((N, 2)).astype(np.float32)
    mask = np.arange(0, N, 3, dtype=np.int32)
    eng = mgn_amd.Engine(9, 3, 2, 128, 2, 2)
    try:
        eng.set_params(orc.init_params(9, 3, 2, 128, 2, 2, 1234, 0.1))
        eng.set_graph(s, r, N)
        train_regime(None, reset=True)
        gs, loss = eng.step(nf, ef, target, mask)
        regime = train_regime(eng, reset=True)
    finally:
        eng.close()
    assert np.isfinite(gs).all() and np.isfinite(loss)
    assert regime["fwd"] == (4, 0, 3, 7) and regime["bwd"] == (4, 0, 3, 7) and regime["lin2"] == (0, 4, 0, 4), regime
    assert regime["factored0"] == 1 and regime["gsets"] == 1 and regime["need_gt"] == 1 and regime["keep_steps"] == 2, regime
    assert regime["rpb_edge0"] == 192 and regime["rpb_node"] == 192, regime
