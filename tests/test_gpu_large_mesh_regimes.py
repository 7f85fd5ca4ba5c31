"""Every large-mesh kernel regime of the processor step on oracle-sized graphs.

Which kernel, block shape and tile walk a launch gets depends on tiles per CU (kernels.hip: num_cus()) and on rounds per wave (frag.hpp:
TileWalk, MGN_SPREAD_ROUNDS).  With the test CU count (mgn_debug_num_cus: C = 8 or 16 instead of the device's 256) a graph of a few
thousand tiles is dispatched exactly as one of 256 / C times its size is on the whole device -- placement is speed only, so 8 blocks must
be as correct as 256 -- and the float64 oracle checks every row of it.  Each case states the family codes that ran
(mgn_debug_last_edge_kernel / mgn_debug_last_node_kernel, table in DESIGN.md), so a moved threshold fails here instead of silently
testing another kernel.

Graphs are ragged (synth.random_graph + hubs): a hub receiver whose run straddles a dozen edge tiles, a second hub in the middle, a block
of receivers without an incoming edge that holds a whole node tile and the last node, a last edge tile of 1, 31 or 32 edges and
N = 1, 31, 0 (mod 32); node 0 is the sender of 40 edges and the receiver of 40.  The hub runs are a few hundred edges, not a third of the graph: an fp32 sum of n terms is off by about
sqrt(n) * 2^-24 of its size, and the per-row bound of 2e-5 must be left to the kernels, not spent on the summation order.

Sizes are written in tiles (T) per test CU (C); the comment of a case names the mesh it stands for on 256 CUs (T / C * 256 tiles x 32)."""
import numpy as np
import pytest
import torch  # noqa: F401  (before the engine's first HIP call)

import mgn_amd
import mgn_oracle as orc
from mgn_amd import synth
from util import (TOL_15, cfg_dict, engine_for, last_kernels, make_params, rel_max, set_fp32_split, set_kernel_path, set_node_ring_hs,
                  set_num_cus, set_renumber, set_ringh_stream, set_split_f16)

pytestmark = pytest.mark.gpu

TILE = 32
ROW_TOL = 2e-5          # per row: max |d| over the row / max |ref| of the row (test_two_fp16_pieces_hold_rows_and_chunks_of_any_scale)
NUM_XCD = 8
SPREAD_ROUNDS = 24      # frag.hpp: MGN_SPREAD_ROUNDS -- per XCD range, from this many rounds of the launch's waves the walk is block-major
NSTEPS = 2
CFG = cfg_dict(mps=NSTEPS)

SETTERS = {"fp32_split": set_fp32_split, "split_f16": set_split_f16, "ringh_stream": set_ringh_stream, "node_ring_hs": set_node_ring_hs,
           "kernel_path": set_kernel_path}


def row_err(a, ref):
    den = np.maximum(np.abs(ref).max(1), 1e-30)
    return float((np.abs(np.asarray(a, np.float64) - ref).max(1) / den).max()) if len(ref) else 0.0


def rows_of(T, tail):
    """rows of T tiles whose last one holds `tail` rows (1, 31 or 32)"""
    return (T - 1) * TILE + tail


_params = None
_graphs = {}
_fp32 = {}


def params():
    global _params
    if _params is None:
        _params = make_params(CFG, jitter=0.05)
    return _params


def graph(N, E):
    """the ragged graph of N nodes and E edges, its latents and the float64 oracle's result: built once, shared, never written to"""
    key = (N, E)
    if key not in _graphs:
        s, r = synth.random_graph(N, E, 7)                        # the last N // 8 nodes receive nothing
        h1, h2 = min(12 * TILE + 5, E // 3), min(70, E // 8)
        r[:h1] = 3                                                # a run over a dozen edge tiles
        r[E // 2: E // 2 + h2] = N // 2                           # a second hub in the middle
        s[E // 4: E // 4 + 40] = 0                                # node 0 sends and receives: row 0 of P / Q is where the kernels park the
        r[3 * (E // 4): 3 * (E // 4) + 40] = 0                    # lanes of rows past N, so a store that loses its guard lands there
        first_empty = N - N // 8
        assert r.max() < first_empty and (first_empty + TILE - 1) // TILE * TILE + TILE <= N   # a whole node tile and the last node: no incoming edge
        rng = np.random.default_rng(N * 1000003 + E)
        v = rng.standard_normal((N, 128)).astype(np.float32)
        e = rng.standard_normal((E, 128)).astype(np.float32)
        rv, re = orc.processor_steps(params(), CFG, v, e, s, r, NSTEPS)
        for a in (s, r, v, e, rv, re):
            a.setflags(write=False)
        _graphs[key] = (s, r, v, e, rv, re)
    return _graphs[key]


class Switches:
    """the CU count and the kernel switches of a case; everything restored on exit"""

    def __init__(self, C, **sw):
        self.C, self.sw, self.old = C, sw, []

    def __enter__(self):
        self.old.append((set_renumber, set_renumber(0)))          # the graph's raggedness is built by node number
        rc = set_num_cus(self.C)
        assert rc == 0, rc                                        # no override was active, and this one was accepted
        self.old.append((set_num_cus, 0))
        for name, val in self.sw.items():
            self.old.append((SETTERS[name], SETTERS[name](val)))
        return self

    def __exit__(self, *exc):
        for fn, val in reversed(self.old):
            fn(val)
        return False


def run(N, E, C, want_engine=False, **sw):
    """The graph through NSTEPS processor steps under the switches, driven call by call the way mgn_processor_steps drives them
    (mgn_proc_begin, then mgn_proc_edge + mgn_proc_node per step) so that the family codes of every step can be read; the one-call
    entry must give the same bits.  Returns (v, e, [(edge code, node code) per step], edge order)."""
    s, r, v, e, _, _ = graph(N, E)
    with Switches(C, **sw):
        eng = engine_for(CFG)
        try:
            eng.set_params(params())
            eng.set_graph(s, r, N)
            eng.latents_import(v, e)
            eng.proc_begin()
            fams = []
            for k in range(NSTEPS):
                eng.proc_edge(k)
                eng.proc_node(k, k + 1 < NSTEPS)
                fams.append(last_kernels())
            v1, e1 = eng.latents_export()
            v2, e2 = eng.processor_steps(v, e, NSTEPS)
            assert np.array_equal(v1, v2) and np.array_equal(e1, e2)
            order = eng.local_edges()                             # engine row j holds input edge order[j]
            if want_engine:
                eng.latents_import(v, e)
                outs = []
                for _ in range(3):
                    eng.latents_import(v, e)
                    eng.processor_steps_dev(NSTEPS)
                    outs.append(eng.latents_export())
                return v1, e1, fams, order, outs
        finally:
            eng.close()
    return v1, e1, fams, order


def fp32_errors(N, E, C):
    """the same graph on the fp32-MFMA kernels (mgn_debug_fp32_split(0)) at the same CU count: its errors against the oracle"""
    key = (N, E, C)
    if key not in _fp32:
        _, _, _, _, rv, re = graph(N, E)
        v0, e0, _, _ = run(N, E, C, fp32_split=0)
        _fp32[key] = max(rel_max(v0, rv), rel_max(e0, re))
    return _fp32[key]


def check(N, E, C, edge_code, node_codes, **sw):
    """assertions 1 - 4 of every case; returns (v, e, edge order) for what a case checks on top"""
    _, _, _, _, rv, re = graph(N, E)
    v1, e1, fams, order = run(N, E, C, **sw)
    node_codes = node_codes if isinstance(node_codes, (list, tuple)) else [node_codes] * NSTEPS
    err = (rel_max(v1, rv), rel_max(e1, re))
    rerr = (row_err(v1, rv), row_err(e1, re))
    print(f"N={N} E={E} C={C} {sw}: families {fams}, rel_max {err[0]:.2e} {err[1]:.2e}, per row {rerr[0]:.2e} {rerr[1]:.2e}")
    assert fams == [(edge_code, n) for n in node_codes], (fams, edge_code, node_codes)     # 1
    assert np.isfinite(v1).all() and np.isfinite(e1).all()
    assert max(err) <= TOL_15, err                                                            # 2
    assert max(rerr) <= ROW_TOL, rerr                                                         # 3
    if sw.get("fp32_split", 1) != 0:                                                          # 4: the split path is no reduced-precision mode
        f32 = fp32_errors(N, E, C)
        print(f"    fp32-MFMA kernels: {f32:.2e}")
        assert max(err) <= 2.0 * f32 + 1e-7, (err, f32)
    return v1, e1, order


def tiles_rows(order, tiles, E):
    return {t: order[t * TILE: min((t + 1) * TILE, E)] for t in tiles}


def walk_edge_tiles(T):
    """the first tile, and the last tile of every XCD's range of the walk (frag.hpp: TileWalk)"""
    per = (T + NUM_XCD - 1) // NUM_XCD
    return sorted({0} | {min((x + 1) * per, T) - 1 for x in range(NUM_XCD) if x * per < T})


def check_edge_tiles(N, E, e1, order, tiles):
    s, r, _, _, _, re = graph(N, E)
    assert np.array_equal(np.sort(order), np.arange(E)) and (np.diff(r[order]) >= 0).all()   # the engine's rows are the edges sorted by receiver
    for t, rows in tiles_rows(order, tiles, E).items():
        err = np.abs(e1[rows].astype(np.float64) - re[rows]).max(1) / np.maximum(np.abs(re[rows]).max(1), 1e-30)
        assert (err <= ROW_TOL).all(), (t, err.max())


# node side of the edge cases: 2 C + 1 tiles -- above two tiles per CU, where the split-path node kernels start
def n_edge_case(C):
    return rows_of(2 * C + 1, 1)


# edge side of the node cases: 12 C tiles (three rounds of four-wave blocks)
def e_node_case(C):
    return rows_of(12 * C, 31)


NODE_DEFAULT = [11, 10]      # k_node_ring_hs (MLP + the next step's P / Q) on every step but the last, which projects nothing: k_node_split_h
C8, C16 = 8, 16


def edge_sizes_1_2_5(C):
    """(tiles, rows of the last tile, what it stands for on 256 CUs) of cases 1, 2 and 5"""
    return [(2 * C + 1, 1, "one partly filled round of four-wave blocks: 513 tiles, 16.4 k edges"),
            (4 * C, 32, "one full round of four-wave blocks: 1 024 tiles, 32.8 k edges"),
            (4 * C + 1, 31, "eight-wave blocks, one round: 1 025 tiles, 32.8 k edges"),
            (8 * C, 32, "eight-wave blocks, one full round: 2 048 tiles, 65.5 k edges"),
            (SPREAD_ROUNDS * NUM_XCD * C, 32, "block-major walk, 24 full rounds: 49 152 tiles, 1.57 M edges"),
            (SPREAD_ROUNDS * NUM_XCD * C + 1, 1, "block-major walk, one tile into the 25th round: 49 153 tiles"),
            (SPREAD_ROUNDS * NUM_XCD * C + 8 * C - 1, 31, "block-major walk, the 25th round one tile short: 51 199 tiles, 1.64 M edges (M-1M: 187 k tiles, the same branch)")]


DEFAULT_EDGE = {0: 17, 1: 17, 2: 16, 3: 16, 4: 16, 5: 16, 6: 16}


@pytest.mark.parametrize("i", range(7))
def test_edge_ring_hs_by_rounds_and_walk(i):
    """cases 1, 2 and 5, default switches: k_edge_ring_hs<4> (17) on one round of four-wave blocks, partly and fully filled,
    k_edge_ring_hs<8> (16) on one round of eight-wave blocks and on the block-major walk -- the non-spread branch of TileWalk, which the
    benchmark's mesh runs and which starts at 192 tiles per CU.  On the block-major sizes the rows of the first tile and of the last
    tile of every XCD's range are compared one by one."""
    T, tail, _ = edge_sizes_1_2_5(C8)[i]
    N, E = n_edge_case(C8), rows_of(T, tail)
    v1, e1, order = check(N, E, C8, DEFAULT_EDGE[i], NODE_DEFAULT)
    if i >= 4:
        check_edge_tiles(N, E, e1, order, walk_edge_tiles(T))


@pytest.mark.parametrize("T_per_C,extra,tail,code", [(8, 1, 1, 17), (12, 0, 32, 17), (40, 3, 31, 16)], ids=["8C+1", "12C", "40C+3"])
def test_edge_ring_hs_several_rounds_spread_walk(T_per_C, extra, tail, code):
    """cases 3 and 4: 8 C + 1 and 12 C tiles run three rounds of four-wave blocks (2 049 and 3 072 tiles on 256 CUs: 65.6 k and 98.3 k
    edges), 40 C + 3 tiles six rounds of eight-wave blocks on the spread walk with a ragged last round (10 243 tiles: 328 k edges)"""
    check(n_edge_case(C8), rows_of(T_per_C * C8 + extra, tail), C8, code, NODE_DEFAULT)


def test_block_major_walk_with_two_blocks_per_xcd():
    """case 5 again at C = 16 (two blocks per XCD label: nb = 2 in TileWalk), the 25th round one tile short: 51 199 tiles on 256 CUs"""
    T = SPREAD_ROUNDS * NUM_XCD * C16 + 8 * C16 - 1
    N, E = n_edge_case(C16), rows_of(T, 31)
    v1, e1, order = check(N, E, C16, 16, NODE_DEFAULT)
    check_edge_tiles(N, E, e1, order, walk_edge_tiles(T))


def node_sizes(C):
    """(node tiles, rows of the last tile, what it stands for on 256 CUs) of cases 6 and 7"""
    return [(2 * C + 1, 1, "seven waves of the third block on padding tiles: 513 tiles, 16.4 k nodes"),
            (8 * C + 1, 31, "one tile into the second round: 2 049 tiles, 65.6 k nodes"),
            (SPREAD_ROUNDS * NUM_XCD * C, 32, "block-major walk, 24 full rounds: 49 152 tiles, 1.57 M nodes"),
            (SPREAD_ROUNDS * NUM_XCD * C + 1, 1, "block-major walk, one tile into the 25th round: 49 153 tiles (M-1M: 31 250 node tiles run the spread walk)")]


@pytest.mark.parametrize("i", range(4))
def test_node_ring_hs_sees_ragged_graphs(i):
    """case 6, default switches: k_node_ring_hs (11).  At 2 C + 1 tiles three blocks are launched and the third holds one tile: its other
    seven waves compute on padding tiles and store nothing."""
    T, tail, _ = node_sizes(C8)[i]
    check(rows_of(T, tail), e_node_case(C8), C8, 17, NODE_DEFAULT)


@pytest.mark.parametrize("i", range(4))
def test_node_split_h_and_project_split_h(i):
    """case 7, mgn_debug_node_ring_hs(0): k_node_split_h (10) and, for the next step's P / Q, k_project_split_h -- what a partitioned run
    launches on its node side"""
    T, tail, _ = node_sizes(C8)[i]
    check(rows_of(T, tail), e_node_case(C8), C8, 17, 10, node_ring_hs=0)


# with mgn_debug_ringh_stream(0) or mgn_debug_split_f16(0) the ring kernels take over from the cooperative tiles above three tiles per CU, not two,
# and run four-wave blocks up to 20 tiles per CU (kernels.hip: launch_edge_step), so the first size of cases 1 / 2 / 5 stays with
# k_edge_coop (3) and the one-round sizes all run four-wave blocks
RING_H_EDGE = {0: 3, 1: 14, 2: 14, 3: 14, 4: 13, 5: 13, 6: 13}
RING_EDGE = {0: 3, 1: 8, 2: 8, 3: 8, 4: 7, 5: 7, 6: 7}


@pytest.mark.parametrize("i", range(7))
def test_edge_ring_h_resident_pieces(i):
    """case 8, mgn_debug_ringh_stream(0): k_edge_ring_h<4 / 8> (14 / 13) at the sizes of cases 1, 2 and 5"""
    T, tail, _ = edge_sizes_1_2_5(C8)[i]
    N, E = n_edge_case(C8), rows_of(T, tail)
    v1, e1, order = check(N, E, C8, RING_H_EDGE[i], NODE_DEFAULT, ringh_stream=0)
    if i >= 4:
        check_edge_tiles(N, E, e1, order, walk_edge_tiles(T))


@pytest.mark.parametrize("i", range(7))
def test_edge_ring_three_bf16_pieces(i):
    """case 9, mgn_debug_split_f16(0): k_edge_ring<4 / 8> (8 / 7) at the sizes of cases 1, 2 and 5; the node side runs k_node_split (5)"""
    T, tail, _ = edge_sizes_1_2_5(C8)[i]
    N, E = n_edge_case(C8), rows_of(T, tail)
    v1, e1, order = check(N, E, C8, RING_EDGE[i], 5, split_f16=0)
    if i >= 4:
        check_edge_tiles(N, E, e1, order, walk_edge_tiles(T))


def test_node_split_three_bf16_pieces():
    """case 9, node side: 8 C + 1 node tiles (2 049 on 256 CUs: 65.6 k nodes) on k_node_split + k_project_split (5)"""
    check(rows_of(8 * C8 + 1, 31), e_node_case(C8), C8, 8, 5, split_f16=0)


@pytest.mark.parametrize("rem_tiles,split", [(5, True), (7 * C8, False)], ids=["tail to k_edge_coop", "whole launch persistent"])
def test_fp32_mfma_persistent_kernels_and_tail_split(rem_tiles, split):
    """case 10, mgn_debug_fp32_split(0): k_edge_step<4, 2> (9) over 24 rounds of 8 C waves plus a last round of 5 tiles, which goes to
    k_edge_coop<false> behind it (49 157 tiles on 256 CUs: 1.57 M edges), or of 7 C tiles, which stays (50 944 tiles); the node side, 8 C + 1
    tiles (2 049: 65.6 k nodes), runs k_node_step (7).  The hand-over shows in results only: the rows before and after it are checked
    apart, and the two tiles at the boundary row by row."""
    T = 8 * C8 * SPREAD_ROUNDS + rem_tiles
    N, E = rows_of(8 * C8 + 1, 1), rows_of(T, 31)
    v1, e1, order = check(N, E, C8, 9, 7, fp32_split=0)
    _, _, _, _, rv, re = graph(N, E)
    body = (T - rem_tiles) * TILE
    rb, rt = order[:body], order[body:]
    assert rel_max(e1[rb], re[rb]) <= TOL_15 and rel_max(e1[rt], re[rt]) <= TOL_15
    check_edge_tiles(N, E, e1, order, [0, T - rem_tiles - 1, T - rem_tiles, T - 1])


@pytest.mark.parametrize("T_per_C,extra,tail", [(2, 1, 1), (4, 0, 32)], ids=["2C+1", "4C"])
def test_fp32_mfma_cooperative_tiles(T_per_C, extra, tail):
    """case 11, mgn_debug_fp32_split(0), kernel_path 0, up to four tiles per CU (513 and 1 024 tiles on 256 CUs): the cooperative four-wave
    tiles with pinned weight rings, k_edge_coop<true> (3) and k_node_coop (3) -- with L = 128 every handle has the t-major fragments, so
    dispatch never reaches the all-streaming k_edge_step<4, 0> (4) at this size"""
    check(n_edge_case(C8), rows_of(T_per_C * C8 + extra, tail), C8, 3, 3, fp32_split=0, kernel_path=0)


# The size thresholds of kernels.hip (struct Switches) that are constants, each with the smallest tile counts on both sides of it where the
# cases above hold only one (the other side is then named in the key).  (node tiles, edge tiles, edge code, node codes, switches) at
# C = 8; tails of 31 / 1 rows on the odd counts.
F32 = dict(fp32_split=0)
THRESHOLDS = {
    "edge coop <= 16C": (2 * C8 + 1, 16 * C8, 3, 3, F32),
    "edge coop > 16C: k_edge_step<4, 2>": (2 * C8 + 1, 16 * C8 + 1, 9, 3, F32),
    "node coop <= 8C": (8 * C8, 2 * C8 + 1, 3, 3, F32),
    "node coop > 8C: k_node_step": (8 * C8 + 1, 2 * C8 + 1, 3, 7, F32),
    "fenced rings <= 4C": (4 * C8, 4 * C8, 3, 3, F32),
    "no fence > 4C": (4 * C8 + 1, 4 * C8 + 1, 3, 3, F32),
    "16-row node kernel behind 32-row edge tiles <= 2C (case 6: 2C + 1)": (2 * C8, 12 * C8, 17, 9, {}),
    "k_edge_ring_hs takes over > 2C: not at 2C (case 1: 2C + 1)": (2 * C8 + 1, 2 * C8, 3, NODE_DEFAULT, {}),
    "k_edge_ring_h takes over > 3C: not at 3C": (2 * C8 + 1, 3 * C8, 3, NODE_DEFAULT, dict(ringh_stream=0)),
    "k_edge_ring_h takes over > 3C": (2 * C8 + 1, 3 * C8 + 1, 14, NODE_DEFAULT, dict(ringh_stream=0)),
    "four waves <= 20C": (2 * C8 + 1, 20 * C8, 14, NODE_DEFAULT, dict(ringh_stream=0)),
    "eight waves > 20C": (2 * C8 + 1, 20 * C8 + 1, 13, NODE_DEFAULT, dict(ringh_stream=0)),
    "k_edge_ring_hs: eight waves at 12C + 1 (case 3: 12C)": (2 * C8 + 1, 12 * C8 + 1, 16, NODE_DEFAULT, {}),
}


@pytest.mark.parametrize("name", list(THRESHOLDS))
def test_family_on_both_sides_of_every_size_threshold(name):
    Tn, Te, edge_code, node_codes, sw = THRESHOLDS[name]
    check(rows_of(Tn, 31 if Tn % 2 else 32), rows_of(Te, 1 if Te % 2 else 32), C8, edge_code, node_codes, **sw)


def test_two_partitions_node_split_h_with_tile_offset():
    """case 12: two partitions of a 48 x 48 mesh in one process (loopback halo exchange), C = 8: 36 node tiles per part (1 152 on 256 CUs:
    36.9 k nodes per part).  Each part runs k_node_split_h (10) over its nodes and k_project_split_h twice, over the boundary tiles and,
    with tile0 != 0, over the interior tiles (> 2 C of them), and the ring edge kernel over the interior and the boundary edge tiles.
    The merged result against the oracle."""
    from importlib import import_module
    halo = import_module("mgn_amd.halo")
    pos, s, r = synth.mesh_1m(9, 48, 48)
    N, E = pos.shape[0], s.size
    rng = np.random.default_rng(12)
    v0 = rng.standard_normal((N, 128)).astype(np.float32)
    e0 = rng.standard_normal((E, 128)).astype(np.float32)
    rv, re = orc.processor_steps(params(), CFG, v0, e0, s, r, NSTEPS)
    stream = torch.cuda.current_stream().cuda_stream
    with Switches(C8):
        engs = []
        try:
            for k in range(2):
                g = engine_for(CFG, rank=k, nranks=2)
                g.set_stream(stream)
                g.set_params(params())
                g.set_graph(s, r, N, mesh_pos=pos)
                g.latents_import(v0, e0)
                engs.append(g)
            for g in engs:
                tb, nt = g.edge_boundary_tiles()
                ntn = (g.n_own + TILE - 1) // TILE
                ntb = (g.boundary_count() + TILE - 1) // TILE
                assert ntn > 2 * C8 and ntn - ntb > 2 * C8 and ntb > 0          # k_node_split_h; k_project_split_h at tile0 = ntb
                assert tb > 0 and nt - tb > 4 * C8                               # interior edge tiles: a ring kernel
            mgn_amd.run_processor_staged(engs, halo.LoopbackExchange(engs, torch.device("cuda")), NSTEPS)
            torch.cuda.synchronize()
            fam = last_kernels()
            v, e = np.zeros((N, 128), np.float32), np.zeros((E, 128), np.float32)
            for g in engs:
                g.latents_export(v, e)
        finally:
            for g in engs:
                g.close()
    err = (rel_max(v, rv), rel_max(e, re))
    print(f"two partitions: families {fam}, rel_max {err}, per row {row_err(v, rv):.2e} {row_err(e, re):.2e}")
    assert fam[0] in (16, 17) and fam[1] == 10, fam
    assert max(err) <= TOL_15, err
    assert max(row_err(v, rv), row_err(e, re)) <= ROW_TOL


@pytest.mark.parametrize("which", ["edge 40C+3", "node 8C+1"])
def test_placement_invariance(which):
    """The same graph at C = 8 and C = 16: the same kernel families, other blocks, other waves per tile range -- and the same bits.  No
    arithmetic depends on which wave owns a tile (no atomics; the aggregate of a receiver is summed in edge order whatever the walk), so
    the two runs must agree exactly; TOL_15 between them is implied."""
    if which.startswith("edge"):
        N, E = n_edge_case(C16), rows_of(40 * C8 + 3, 31)       # (node tiles above two per CU at both counts)
        fam = [(16, 11), (16, 10)]
    else:
        N, E = rows_of(8 * C8 + 1, 31), rows_of(40 * C8 + 3, 31)  # (an edge side that runs eight-wave blocks at both counts)
        fam = [(16, 11), (16, 10)]
    va, ea, fa, _ = run(N, E, C8)
    vb, eb, fb, _ = run(N, E, C16)
    assert fa == fam and fb == fam, (fa, fb)
    print("placement:", which, rel_max(vb, va), rel_max(eb, ea))
    assert rel_max(vb, va) <= TOL_15 and rel_max(eb, ea) <= TOL_15
    assert np.array_equal(va, vb) and np.array_equal(ea, eb)


def test_block_major_pass_is_bitwise_repeatable():
    """case 5's largest graph three times through mgn_processor_steps_dev: equal bits (test_processor_pass_is_bitwise_repeatable runs
    spread-walk sizes only)"""
    T = SPREAD_ROUNDS * NUM_XCD * C8 + 8 * C8 - 1
    N, E = n_edge_case(C8), rows_of(T, 31)
    v1, e1, fams, _, outs = run(N, E, C8, want_engine=True)
    assert fams == [(16, 11), (16, 10)], fams
    for v, e in outs:
        assert np.array_equal(v, v1) and np.array_equal(e, e1)


def test_cu_count_is_validated_and_no_override_is_left():
    """mgn_debug_num_cus takes multiples of 8 from 8 up to the device's count and nothing else; after this module (and whatever ran
    before it) no override is active"""
    assert set_num_cus(0) == 0
    dev = torch.cuda.get_device_properties(0).multi_processor_count
    for bad in (-8, 1, 4, 12, dev + 8):
        assert set_num_cus(bad) == -1
        assert set_num_cus(0) == 0
    assert set_num_cus(8) == 0 and set_num_cus(16) == 8 and set_num_cus(0) == 16 and set_num_cus(0) == 0
