"""The case graphs of the bf16 regime tests and their references (test infrastructure; numpy and the oracle only, no GPU).

tests/test_gpu_bf16_regimes.py runs the kernels on these graphs, tests/test_bf16_model_host.py checks on the CPU that the bounds the GPU
file asserts can see the faults they are there for.  Everything here is built once per graph, shared and never written to.

Graph (N nodes, E edges): synth.random_graph(N, E, 7) with latents from standard_normal; the engine's rows are the edges sorted by
receiver (one partition, no renumbering), and the hubs are placed in that order so that every piece of their aggregates matters:
  * node 0 receives the first 40 rows (pieces 32 + 8; tile 0 has no tile before it) and sends 40 edges -- row 0 of P / Q is where the
    kernels park the lanes of invalid rows;
  * hub runs of 40, 80, 108 and 144 rows that begin 30, 24, 20 and 8 rows into a 32-row tile: pieces 2 + 32 + 6 (a whole tile of one
    receiver, a 2-edge piece), 8 + 32 + 32 + 8, 12 + 32 + 32 + 32 (ends on a tile boundary) and 24 + 3 x 32 + 24 (five pieces; the node
    kernel's loop over third and later carry rows runs from three pieces on).  Graphs under 1 500 edges hold the first two, under 500
    the first only.  Longer runs or shorter end pieces do not pass the sensitivity conditions of tests/test_bf16_model_host.py: a
    dropped end piece of 3 or 4 rows of a run of 70 or 100 moved its node's row by 1.3 x bound 3, 16 rows of 170 (six pieces) by 1.1 x,
    28 rows of 184 (six pieces) by 1.2 x, against the 1.5 x required -- the aggregate of a long run barely turns when a piece is lost;
  * the nodes from the start of the next-to-last node tile on, and at least the last N // 8, receive nothing: a whole node tile and
    the last node;
  * no run is longer than a few hundred edges (the reason tests/test_gpu_large_mesh_regimes.py gives)."""
import numpy as np

import mgn_oracle as orc
from mgn_amd import synth

TILE = 32
NSTEPS = 2
CFG = dict(Fn=9, Fe=3, O=2, L=128, hidden_layers=2, mps=NSTEPS)
CFG2 = dict(Fn=9, Fe=3, O=2, L=128, hidden_layers=2, mps=NSTEPS, Fe2=4)
HUBS = [(40, 30, 3), (80, 24, 4), (108, 20, 4), (144, 8, 5)]      # (rows, rows into its first tile, pieces)


def rows_of(T, tail):
    """rows of T tiles whose last one holds `tail` rows (1, 31 or 32)"""
    return (T - 1) * TILE + tail


def row_rel(a, ref):
    """relative L2 error of every row"""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return np.linalg.norm(a - ref, axis=1) / np.maximum(np.linalg.norm(ref, axis=1), 1e-30)


def rel_l2(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm(a - ref) / max(np.linalg.norm(ref), 1e-30))


def rmax(x):
    return float(x.max()) if x.size else 0.0


_params = {}


def params(cfg=CFG):
    key = tuple(sorted(cfg.items()))
    if key not in _params:
        _params[key] = orc.init_params(cfg["Fn"], cfg["Fe"], cfg["O"], cfg["L"], 2, cfg["mps"], 1234, 0.05, Fe2=cfg.get("Fe2"))
        _params[key].setflags(write=False)
    return _params[key]


def hubs_for(E):
    return HUBS if E >= 1500 else HUBS[:2] if E >= 500 else HUBS[:1]


def ragged(N, E):
    """(senders, receivers, {hub node: (first engine row, rows)}) of the case graph"""
    s, r = synth.random_graph(N, E, 7)
    first_empty = min(N - N // 8, ((N - 1) // TILE - 1) * TILE)
    assert first_empty > 64
    order0 = np.argsort(r % first_empty, kind="stable")
    rs = (r % first_empty)[order0]                                 # the engine's rows: receivers in ascending order
    end0 = int(np.searchsorted(rs, 0, "right"))
    if end0 > 40:
        rs[40:end0] = rs[end0]                                     # (dense graphs: node 0 keeps 40 of its edges)
    rs[:40] = 0
    hubs = hubs_for(E)
    lo0 = 2 * TILE
    span = (E - lo0) // len(hubs)
    placed = {}
    for k, (rows, off, _) in enumerate(hubs):
        lo, hi = lo0 + k * span, lo0 + (k + 1) * span
        p0 = lo + TILE + (off - lo) % TILE                          # the first row >= lo + TILE that lies `off` rows into a tile
        assert p0 + rows + 1 < hi, (N, E, k)
        e1 = int(np.searchsorted(rs, rs[p0 - 1], "right"))          # the hub is the first receiver after the one that holds row p0 - 1,
        h = int(rs[e1])                                            # whose run ends at p0 now
        end = max(int(np.searchsorted(rs, h, "right")), p0 + rows)
        rs[p0 + rows:end] = rs[end]                                # what is left of the two runs goes to the next receiver
        rs[p0:p0 + rows] = h
        placed[h] = (p0, rows)
    for h, (p0, rows) in placed.items():
        assert h and np.searchsorted(rs, h, "left") == p0 and np.searchsorted(rs, h, "right") == p0 + rows, (N, E, h)
    assert (np.diff(rs) >= 0).all() and rs.max() < first_empty
    r[order0] = rs
    s[E // 4: E // 4 + 40] = 0
    return s, r, placed


class Ref:
    """A case graph, its latents and the three references after every step: the float64 oracle, the bf16 model with float64 sums and
    with float32 sums.  spread[k] = (v, e): the largest per-row relative L2 between the two models after step k + 1 -- bound 3 is twice
    that; model_err[k] = (v, e, v global, e global): the model against the oracle -- bound (a) is twice that."""


_refs = {}


def reference(N, E, mode="mfma", nsteps=NSTEPS):
    key = (N, E, mode, nsteps)
    if key in _refs:
        return _refs[key]
    g = Ref()
    g.N, g.E, g.mode, g.tile_rows = N, E, mode, (16 if mode == "storage" else TILE)
    g.s, g.r, g.hubs = ragged(N, E)
    rng = np.random.default_rng(N * 1000003 + E)
    g.v = rng.standard_normal((N, 128)).astype(np.float32)
    g.e = rng.standard_normal((E, 128)).astype(np.float32)
    g.order = np.argsort(g.r, kind="stable")                      # == Engine.local_edges() (asserted by the GPU tests)
    fill(g, CFG, nsteps)
    _refs[key] = g
    return g


def fill(g, cfg, nsteps, set2=None):
    """the three references of g (set2 = (e2, s2, r2, order2))"""
    ps = params(cfg)
    o2 = None if set2 is None else set2[:3]
    g.orc, P = [], orc._unpack(ps, cfg, np.float64)
    state = (np.asarray(g.v, np.float64), np.asarray(g.e, np.float64)) + (() if set2 is None else (np.asarray(set2[0], np.float64),))
    for k in range(nsteps):
        state = orc.processor_step(P, k, state[0], state[1], g.s, g.r, 2, None if set2 is None else (state[2], o2[1], o2[2]))
        g.orc.append(state)
    kw = dict(tile_rows=g.tile_rows, mode=g.mode, set2=set2, all_steps=True)
    g.m64 = orc.processor_steps_bf16(ps, cfg, g.v, g.e, g.s, g.r, nsteps, g.order, acc=np.float64, **kw)
    g.m32 = orc.processor_steps_bf16(ps, cfg, g.v, g.e, g.s, g.r, nsteps, g.order, acc=np.float32, **kw)
    g.spread = [tuple(rmax(row_rel(a, b)) for a, b in zip(g.m32[k], g.m64[k])) for k in range(nsteps)]
    g.model_err = [tuple(rmax(row_rel(a, b)) for a, b in zip(g.m64[k], g.orc[k])) + tuple(rel_l2(a, b) for a, b in zip(g.m64[k], g.orc[k]))
                   for k in range(nsteps)]
    for arrs in (g.orc, g.m64, g.m32):
        for st in arrs:
            for a in st:
                a.setflags(write=False)
    for a in (g.s, g.r, g.v, g.e, g.order):
        a.setflags(write=False)


def reference_two_sets(N, E, E2):
    key = (N, E, E2)
    if key in _refs:
        return _refs[key]
    g = Ref()
    g.N, g.E, g.E2, g.mode, g.tile_rows = N, E, E2, "mfma", TILE
    g.s, g.r, g.hubs = ragged(N, E)
    g.s2, g.r2, g.hubs2 = ragged(N, E2)
    g.s2 = np.roll(g.s2, 7)                                        # (not the first set's senders again)
    rng = np.random.default_rng(N * 1000003 + E + E2)
    g.v = rng.standard_normal((N, 128)).astype(np.float32)
    g.e = rng.standard_normal((E, 128)).astype(np.float32)
    g.e2 = rng.standard_normal((E2, 128)).astype(np.float32)
    g.order = np.argsort(g.r, kind="stable")
    g.order2 = np.argsort(g.r2, kind="stable")
    fill(g, CFG2, NSTEPS, set2=(g.e2, g.s2, g.r2, g.order2))
    _refs[key] = g
    return g


def reference_mesh(nx, ny, seed=9):
    """a triangle mesh (the two-partition case): references in the single partition's edge order"""
    key = ("mesh", nx, ny, seed)
    if key in _refs:
        return _refs[key]
    g = Ref()
    g.pos, g.s, g.r = synth.mesh_1m(seed, nx, ny)
    g.N, g.E, g.mode, g.tile_rows, g.hubs = g.pos.shape[0], g.s.size, "mfma", TILE, {}
    rng = np.random.default_rng(12)
    g.v = rng.standard_normal((g.N, 128)).astype(np.float32)
    g.e = rng.standard_normal((g.E, 128)).astype(np.float32)
    g.order = np.argsort(g.r, kind="stable")
    fill(g, CFG, NSTEPS)
    _refs[key] = g
    return g


C8, C16 = 8, 16
NUM_XCD = 8
SPREAD_ROUNDS = 24      # frag.hpp: MGN_SPREAD_ROUNDS
PIPE = (18, 12)         # k_edge_bf16_pipe, k_node_bf16_pipe
C16_CODES = (15, 8)     # k_edge_coop16m on two fp16 pieces, k_node_coop16 on the split path: the 16-row kernels on the bf16 arrays

# id: (node tiles, rows of the last node tile, edge tiles, rows of the last edge tile, test CU count, kernel path, model mode, codes)
# T tiles on C test CUs are dispatched as T / C * 256 tiles are on the whole device.
CASES = {
    # hand-over between the 16-row kernels (carry rows per 16-edge tile) and the pipe kernels (per 32-edge tile): use_c16 holds up to
    # C node tiles and 3 C edge tiles
    "handover 16-row":    (C8, 32, 3 * C8, 31, C8, 0, "storage", C16_CODES),
    "handover node C+1":  (C8 + 1, 1, 3 * C8, 32, C8, 0, "mfma", PIPE),       # node launch: 2 waves per block
    "handover edge 3C+1": (C8, 31, 3 * C8 + 1, 1, C8, 0, "mfma", PIPE),      # edge launch: 4 waves per block; node launch: 1 wave
    # waves per block (tile_launch: 1 / 2 / 4 / 8 up to C / 2 C / 4 C tiles and above)
    "edge 4C+1":          (2 * C8 + 1, 31, 4 * C8 + 1, 31, C8, 0, "mfma", PIPE),  # 8 waves, a partly filled round; node launch: 4 waves
    "edge C path 1":      (C8 + 1, 32, C8, 32, C8, 1, "mfma", PIPE),          # 1 wave per block
    "edge C+1 path 1":    (C8, 1, C8 + 1, 1, C8, 1, "mfma", PIPE),            # 2 waves, XCD ranges 5 .. 7 get no tile
    # tiles per wave of the software pipeline (8 C waves): 1, 2, 3, 4, and unequal counts per wave and per XCD
    "edge 8C":            (4 * C8 + 1, 1, 8 * C8, 32, C8, 0, "mfma", PIPE),       # node launch: 8 waves
    "edge 16C":           (2 * C8 + 1, 1, 16 * C8, 31, C8, 0, "mfma", PIPE),
    "edge 24C":           (2 * C8 + 1, 1, 24 * C8, 32, C8, 0, "mfma", PIPE),
    "edge 32C":           (2 * C8 + 1, 1, 32 * C8, 1, C8, 0, "mfma", PIPE),
    "edge 24C+1":         (2 * C8 + 1, 1, 24 * C8 + 1, 31, C8, 0, "mfma", PIPE),
    "edge 40C+3":         (2 * C8 + 1, 1, 40 * C8 + 3, 31, C8, 0, "mfma", PIPE),
    # the walk (frag.hpp: TileWalk): block-major from per = ceil(T / 8) >= 24 x the launch's waves per XCD label
    "walk 192C-8":        (2 * C8 + 1, 1, SPREAD_ROUNDS * NUM_XCD * C8 - 8, 32, C8, 0, "mfma", PIPE),     # per = 24 C - 1: the last wave-major size
    "walk 192C-1":        (2 * C8 + 1, 1, SPREAD_ROUNDS * NUM_XCD * C8 - 1, 31, C8, 0, "mfma", PIPE),
    "walk 192C+1":        (2 * C8 + 1, 1, SPREAD_ROUNDS * NUM_XCD * C8 + 1, 1, C8, 0, "mfma", PIPE),
    "walk 192C-1 C16":    (2 * C16 + 1, 1, SPREAD_ROUNDS * NUM_XCD * C16 - 1, 31, C16, 0, "mfma", PIPE),  # two blocks per XCD label
    "walk 192C+1 C16":    (2 * C16 + 1, 1, SPREAD_ROUNDS * NUM_XCD * C16 + 1, 1, C16, 0, "mfma", PIPE),
}
WALK_CASES = [k for k in CASES if k.startswith("walk")]
TWO_SETS = (2 * C8 + 1, 1, 8 * C8 + 1, 31, 3 * C8 + 1, 1)         # node tiles, tail, set 1 tiles, tail, set 2 tiles, tail


def case_ref(name):
    Tn, tn, Te, te, C, path, mode, codes = CASES[name]
    return reference(rows_of(Tn, tn), rows_of(Te, te), mode)


def hub_pieces(g, tile_rows=None):
    """{hub node: indices of its pieces in edge_pieces(...)} and (starts, receivers) of all pieces"""
    starts, pr = orc.edge_pieces(g.r, g.order, tile_rows or g.tile_rows)
    return {h: np.nonzero(pr == h)[0] for h in g.hubs}, starts, pr
