"""Every regime of the bf16 processor kernels against a per-row model, the way tests/test_gpu_large_mesh_regimes.py holds the fp32 kernels.

k_edge_bf16_pipe, k_node_bf16_pipe and k_project_bf16_pipe take their block shape from tiles per CU (kernels.hip: tile_launch -- 1 / 2 / 4 / 8
waves per block), their tile walk from rounds per wave (frag.hpp: TileWalk) and hand small graphs to the 16-row kernels (mgn_api.cpp:
use_c16, where the carry rows change from 16-edge to 32-edge tiles).  With the test CU count (mgn_debug_num_cus: C = 8 or 16) each of
these branches exists on a graph the CPU can check.  Each case asserts

  1. the family codes of every step (18 k_edge_bf16_pipe, 12 k_node_bf16_pipe; the 16-row kernels 15 / 8),
  2. finite results; the same bits from the call-by-call drive, from mgn_processor_steps and from three mgn_processor_steps_dev passes,
  3. per row, after step 1 and after step 2: relative L2 against the bf16 rounding model of the oracle
     (mgn_oracle.processor_steps_bf16, float64 sums) <= 2 x the largest per-row relative L2 between that model with float32 sums and
     with float64 sums, over the same array and step.  The two model runs differ where an fp32-level difference flips a bf16 rounding;
     the MFMA summation order is a third sample of the same thing, hence the factor 2.  Nothing is hard-coded,
  4. per row against the float64 oracle <= 2 x the model's own largest per-row error (bound (a)); globally <= 2 x the model's own.

The graphs, the cases and the references are in tests/bf16_cases.py; tests/test_bf16_model_host.py shows on the CPU that bound 3 sees
a lost piece, exchanged carry rows, a neighbour's aggregate, a lost edge row and a lost residual on every one of these graphs.

Measured on an MI355X (largest per-row relative L2 over v and e; bound 3 = 2 x spread, bound (a) = 2 x model error):

(all figures x 1e-3; v / e [/ e2]; N, E and the codes of both steps first)
case                     N       E codes    step  to the model  (bound 3)      to the oracle  (bound (a))      global  (2 x model)
handover 16-row        256     767 15 / 8   1     0.6 / 0.1     (4.2 / 3.2)    3.6 / 3.5      (7.2 / 7.1)    2.5 / 2.6  (5.0 / 5.1)
handover 16-row        256     767 15 / 8   2     2.3 / 1.4     (6.2 / 5.1)    4.6 / 4.4      (9.1 / 8.8)    3.1 / 3.1  (6.3 / 6.3)
handover node C+1      257     768 18 / 12  1     3.5 / 2.0     (5.4 / 4.0)    6.0 / 5.4      (12.0 / 10.8)    4.1 / 3.7  (8.1 / 7.4)
handover node C+1      257     768 18 / 12  2     4.8 / 4.0     (8.3 / 8.0)    8.7 / 7.0      (17.3 / 14.1)    5.3 / 4.7  (10.6 / 9.4)
handover edge 3C+1     255     769 18 / 12  1     2.0 / 1.3     (4.0 / 2.6)    6.5 / 5.4      (13.0 / 10.8)    4.1 / 3.7  (8.2 / 7.4)
handover edge 3C+1     255     769 18 / 12  2     3.3 / 3.1     (6.6 / 6.3)    7.6 / 7.1      (15.2 / 14.2)    5.2 / 4.7  (10.4 / 9.3)
edge 4C+1              543    1055 18 / 12  1     2.7 / 1.0     (5.4 / 2.2)    8.0 / 5.4      (16.0 / 10.7)    4.1 / 3.7  (8.2 / 7.3)
edge 4C+1              543    1055 18 / 12  2     5.3 / 3.3     (9.1 / 7.0)    8.2 / 6.8      (16.3 / 13.6)    5.3 / 4.7  (10.6 / 9.4)
edge C path 1          288     256 18 / 12  1     3.4 / 2.3     (7.8 / 4.8)    6.2 / 5.0      (12.5 / 10.1)    3.8 / 3.8  (7.7 / 7.5)
edge C path 1          288     256 18 / 12  2     4.9 / 4.1     (10.8 / 7.4)    7.6 / 6.6      (15.2 / 13.1)    5.1 / 4.9  (10.2 / 9.7)
edge C+1 path 1        225     257 18 / 12  1     1.6 / 0.2     (3.2 / 1.0)    6.1 / 4.7      (12.2 / 9.4)    3.8 / 3.6  (7.6 / 7.2)
edge C+1 path 1        225     257 18 / 12  2     3.7 / 2.4     (8.2 / 5.7)    7.5 / 6.0      (15.0 / 12.1)    5.0 / 4.6  (10.0 / 9.3)
edge 8C               1025    2048 18 / 12  1     3.9 / 3.1     (7.8 / 6.1)    6.2 / 5.6      (12.4 / 11.2)    4.0 / 3.7  (8.1 / 7.4)
edge 8C               1025    2048 18 / 12  2     5.6 / 4.4     (11.1 / 8.7)    8.4 / 6.8      (16.7 / 13.7)    5.3 / 4.7  (10.5 / 9.4)
edge 16C               513    4095 18 / 12  1     2.9 / 2.3     (3.6 / 2.9)    6.6 / 6.0      (13.1 / 12.1)    4.2 / 3.7  (8.5 / 7.4)
edge 16C               513    4095 18 / 12  2     4.4 / 4.5     (7.3 / 6.6)    7.5 / 7.4      (14.9 / 14.8)    5.2 / 4.7  (10.4 / 9.4)
edge 24C               513    6144 18 / 12  1     3.0 / 2.4     (6.1 / 3.4)    6.3 / 5.8      (12.6 / 11.6)    4.2 / 3.7  (8.4 / 7.4)
edge 24C               513    6144 18 / 12  2     4.4 / 4.0     (8.5 / 8.2)    7.7 / 7.5      (15.4 / 14.9)    5.2 / 4.7  (10.3 / 9.4)
edge 32C               513    8161 18 / 12  1     3.6 / 2.9     (6.6 / 5.9)    6.3 / 5.9      (12.6 / 11.8)    4.2 / 3.7  (8.5 / 7.4)
edge 32C               513    8161 18 / 12  2     4.7 / 4.7     (9.1 / 9.3)    7.9 / 7.1      (16.0 / 14.2)    5.2 / 4.7  (10.3 / 9.4)
edge 24C+1             513    6175 18 / 12  1     3.1 / 2.6     (6.6 / 7.0)    7.0 / 5.6      (14.0 / 11.3)    4.2 / 3.7  (8.4 / 7.4)
edge 24C+1             513    6175 18 / 12  2     4.7 / 4.2     (9.9 / 9.4)    7.6 / 7.5      (15.3 / 15.0)    5.2 / 4.7  (10.3 / 9.4)
edge 40C+3             513   10335 18 / 12  1     3.4 / 3.1     (7.4 / 6.0)    6.8 / 5.8      (13.6 / 11.7)    4.3 / 3.7  (8.6 / 7.4)
edge 40C+3             513   10335 18 / 12  2     4.8 / 4.3     (9.2 / 8.4)    7.9 / 7.9      (15.7 / 15.9)    5.2 / 4.7  (10.5 / 9.4)
walk 192C-8            513   48896 18 / 12  1     3.1 / 3.2     (7.5 / 6.0)    6.4 / 6.0      (12.8 / 12.1)    4.2 / 3.7  (8.4 / 7.4)
walk 192C-8            513   48896 18 / 12  2     4.9 / 4.6     (9.4 / 9.2)    7.0 / 7.6      (14.0 / 15.2)    5.1 / 4.7  (10.2 / 9.3)
walk 192C-1            513   49119 18 / 12  1     3.4 / 2.9     (6.3 / 5.2)    5.9 / 6.1      (11.8 / 12.3)    4.2 / 3.7  (8.3 / 7.4)
walk 192C-1            513   49119 18 / 12  2     5.0 / 4.5     (9.1 / 8.7)    6.9 / 7.7      (13.7 / 15.5)    5.1 / 4.7  (10.2 / 9.3)
walk 192C+1            513   49153 18 / 12  1     3.7 / 3.2     (7.3 / 6.3)    5.9 / 6.3      (11.7 / 12.6)    4.2 / 3.7  (8.3 / 7.4)
walk 192C+1            513   49153 18 / 12  2     5.3 / 4.4     (10.0 / 10.4)    6.8 / 7.9      (13.6 / 15.8)    5.1 / 4.7  (10.2 / 9.4)
walk 192C-1 C16       1025   98271 18 / 12  1     3.7 / 3.6     (7.4 / 6.5)    5.8 / 6.5      (11.7 / 13.0)    4.2 / 3.7  (8.3 / 7.4)
walk 192C-1 C16       1025   98271 18 / 12  2     4.9 / 4.7     (9.3 / 9.9)    7.5 / 7.7      (15.1 / 15.3)    5.1 / 4.7  (10.1 / 9.4)
walk 192C+1 C16       1025   98305 18 / 12  1     3.6 / 3.7     (7.7 / 6.0)    5.9 / 6.4      (12.0 / 12.8)    4.2 / 3.7  (8.3 / 7.4)
walk 192C+1 C16       1025   98305 18 / 12  2     5.1 / 4.7     (10.2 / 8.8)    7.6 / 8.1      (15.1 / 16.2)    5.1 / 4.7  (10.2 / 9.4)
two edge sets          513    2079 18 / 12  1     0.5 / 0.5 / 0.1(6.1 / 2.9 / 1.0)    6.6 / 5.4 / 5.2 (13.3 / 10.8 / 10.5)    4.1 / 3.7 / 3.6  (8.2 / 7.5 / 7.2)
two edge sets          513    2079 18 / 12  2     3.1 / 3.2 / 1.8(9.2 / 7.6 / 6.0)    7.9 / 6.9 / 7.0 (15.8 / 13.9 / 13.9)    5.1 / 4.8 / 4.7  (10.2 / 9.6 / 9.3)
two partitions        2304   13442 18 / 12  2     - / -         (- / -)    9.0 / 7.8      (15.8 / 15.6)    5.4 / 4.7  (10.9 / 9.4)
plain preload        16353  524319 18 / 12  1     4.5 / 4.5     (8.4 / 8.9)    7.3 / 6.7      (14.6 / 13.4)    4.3 / 3.7  (8.5 / 7.4)
"""
import numpy as np
import pytest
import torch  # noqa: F401  (before the engine's first HIP call)

import bf16_cases as bc
import mgn_amd
from bf16_cases import C8, CASES, NSTEPS, NUM_XCD, TILE, WALK_CASES, rel_l2, rmax, row_rel, rows_of
from util import engine_for, last_kernels, set_kernel_path, set_num_cus, set_renumber

pytestmark = pytest.mark.gpu


class Switches:
    """the CU count and the kernel path of a case; everything restored on exit"""

    def __init__(self, C, path=0):
        self.C, self.path, self.old = C, path, []

    def __enter__(self):
        self.old.append((set_renumber, set_renumber(0)))          # the graph's raggedness is built by node number
        rc = set_num_cus(self.C)
        assert rc == 0, rc                                        # no override was active, and this one was accepted
        self.old.append((set_num_cus, 0))
        self.old.append((set_kernel_path, set_kernel_path(self.path)))
        return self

    def __exit__(self, *exc):
        for fn, val in reversed(self.old):
            fn(val)
        return False


def drive(eng, g, nsteps, e2=None):
    """nsteps processor steps call by call (mgn_proc_begin, then mgn_proc_edge + mgn_proc_node per step), the latents exported and the
    family codes read after every step; then the one-call entries, which must give the same bits"""
    def put():
        eng.latents_import(g.v, g.e)
        if e2 is not None:
            eng.edge_latents_import(1, e2)

    def get():
        return eng.latents_export() + (() if e2 is None else (eng.edge_latents_export(1),))

    put()
    eng.proc_begin()
    steps, fams = [], []
    for k in range(nsteps):
        eng.proc_edge(k)
        eng.proc_node(k, k + 1 < nsteps)
        fams.append(last_kernels())
        steps.append(get())
    if e2 is None:
        for n in range(1, nsteps + 1):
            vn, en = eng.processor_steps(g.v, g.e, n)
            assert np.array_equal(vn, steps[n - 1][0]) and np.array_equal(en, steps[n - 1][1]), n
    for _ in range(3):
        put()
        eng.processor_steps_dev(nsteps)
        for a, b in zip(get(), steps[-1]):
            assert np.array_equal(a, b)
    return steps, fams


def assert_bounds(label, g, steps, first_step=0):
    """assertions 2 - 4 of the results after every step, figures printed first"""
    names = ("v", "e", "e2")
    fails = []
    for k in range(first_step, len(steps)):
        got = steps[k]
        nar = len(got)
        assert all(np.isfinite(a).all() for a in got)
        for i in range(nar):
            to_model, to_orc = rmax(row_rel(got[i], g.m64[k][i])), rmax(row_rel(got[i], g.orc[k][i]))
            glob = rel_l2(got[i], g.orc[k][i])
            b3, ba, bg = 2.0 * g.spread[k][i], 2.0 * g.model_err[k][i], 2.0 * g.model_err[k][nar + i]
            print(f"    {label} step {k + 1} {names[i]}: per row to the model {to_model:.2e} (bound 3 {b3:.2e}), to the oracle {to_orc:.2e} "
                  f"(bound (a) {ba:.2e}), global {glob:.2e} (<= {bg:.2e})")
            if not to_model <= b3:
                fails.append((k + 1, names[i], "bound 3", to_model, b3))
            if not to_orc <= ba:
                fails.append((k + 1, names[i], "bound (a)", to_orc, ba))
            if not glob <= bg:
                fails.append((k + 1, names[i], "global", glob, bg))
    assert not fails, fails


def run_case(name):
    Tn, tn, Te, te, C, path, mode, codes = CASES[name]
    g = bc.case_ref(name)
    with Switches(C, path):
        eng = engine_for(bc.CFG, dtype="bf16")
        try:
            eng.set_params(bc.params())
            eng.set_graph(g.s, g.r, g.N)
            assert np.array_equal(eng.local_edges(), g.order)     # engine row j holds input edge order[j]: the model's pieces are the kernels'
            steps, fams = drive(eng, g, NSTEPS)
        finally:
            eng.close()
    print(f"{name}: N={g.N} E={g.E} C={C} path {path}: families {fams}")
    assert fams == [codes] * NSTEPS, (fams, codes)                                            # 1
    assert_bounds(name, g, steps)                                                             # 2 - 4
    return g, steps


HANDOVER = [n for n in CASES if n.startswith("handover")]
WAVES = ["edge 4C+1", "edge C path 1", "edge C+1 path 1"]
PER_WAVE = ["edge 8C", "edge 16C", "edge 24C", "edge 32C", "edge 24C+1", "edge 40C+3"]
assert sorted(HANDOVER + WAVES + PER_WAVE + WALK_CASES) == sorted(CASES)


@pytest.mark.parametrize("name", HANDOVER)
def test_handover_between_the_16_row_and_the_pipe_kernels(name):
    """C node tiles and 3 C edge tiles run the 16-row kernels on the bf16 arrays (carry rows per 16-edge tile: the model's "storage" mode);
    one node tile or one edge tile more and both launches are the pipe kernels (carry rows per 32-edge tile).  Node launches of 1 and
    2 waves per block, an edge launch of 4."""
    Tn, tn, Te, te, C, path, mode, codes = CASES[name]
    assert (Tn <= C and Te <= 3 * C) == (mode == "storage")
    run_case(name)


@pytest.mark.parametrize("name", WAVES)
def test_waves_per_block(name):
    """4 C + 1 edge tiles: eight-wave blocks, a partly filled round (node side 2 C + 1 tiles: four waves); under kernel path 1 the pipe
    kernels run at any size: C and C + 1 edge tiles give one and two waves per block, and XCD ranges without a tile"""
    run_case(name)


@pytest.mark.parametrize("name", PER_WAVE)
def test_tiles_per_wave_of_the_pipeline(name):
    """8 C, 16 C, 24 C and 32 C edge tiles are 1, 2, 3 and 4 tiles per wave -- the prologue alone, both exits of the loop of
    k_edge_bf16_pipe (more1 / more2: odd and even counts), the two e buffers and the ix / ixn / ixnn hand-over in every position;
    24 C + 1 and 40 C + 3 give unequal counts per wave and per XCD (clampt past a wave's last tile).  8 C has 4 C + 1 node tiles:
    eight-wave node and project launches."""
    run_case(name)


def walk_edge_tiles(T):
    """the first tile, and the last tile of every XCD's range of the walk (frag.hpp: TileWalk)"""
    per = (T + NUM_XCD - 1) // NUM_XCD
    return sorted({0} | {min((x + 1) * per, T) - 1 for x in range(NUM_XCD) if x * per < T})


@pytest.mark.parametrize("name", WALK_CASES)
def test_walk_on_both_sides_of_the_spread_rounds(name):
    """TileWalk numbers a wave's positions block-major from per = ceil(T / 8) >= 24 x (waves per XCD label): 192 C - 8 tiles are the
    last wave-major size, 192 C - 1 and 192 C + 1 block-major with a last round one tile short and one tile long (the benchmark's mesh:
    187 k tiles, the same branch).  At C = 16 an XCD label has two blocks, the only place the two numberings differ.  The first tile and
    the last tile of every XCD's range are checked row by row on top."""
    Tn, tn, Te, te, C, path, mode, codes = CASES[name]
    per, stride = (Te + NUM_XCD - 1) // NUM_XCD, C // NUM_XCD * 8
    assert (per < bc.SPREAD_ROUNDS * stride) == name.startswith("walk 192C-8")
    g, steps = run_case(name)
    for k in range(NSTEPS):
        for t in walk_edge_tiles(Te):
            rows = g.order[t * TILE: min((t + 1) * TILE, g.E)]
            err = row_rel(steps[k][1][rows], g.m64[k][1][rows])
            assert (err <= 2.0 * g.spread[k][1]).all(), (k, t, err.max())
            assert (row_rel(steps[k][1][rows], g.e[rows]) > 0.1).all()         # every row of the tile was computed


def test_two_edge_sets_reach_the_second_aggregate():
    """the AGG2 / chunk[6] branch of k_node_bf16_pipe: sets of 8 C + 1 and 3 C + 1 tiles, each with its hubs"""
    Tn, tn, T1, t1, T2, t2 = bc.TWO_SETS
    g = bc.reference_two_sets(rows_of(Tn, tn), rows_of(T1, t1), rows_of(T2, t2))
    cfg = bc.CFG2
    with Switches(C8):
        eng = mgn_amd.Engine(cfg["Fn"], cfg["Fe"], cfg["O"], cfg["L"], 2, cfg["mps"], Fe2=cfg["Fe2"], dtype="bf16")
        try:
            eng.set_params(bc.params(cfg))
            eng.set_graph(g.s, g.r, g.N)
            eng.set_edge_set(1, g.s2, g.r2)
            assert np.array_equal(eng.local_edges(), g.order)
            steps, fams = drive(eng, g, NSTEPS, e2=g.e2)
        finally:
            eng.close()
    print(f"two edge sets: N={g.N} E={g.E} E2={g.E2}: families {fams}")
    assert fams == [bc.PIPE] * NSTEPS, fams
    assert_bounds("two edge sets", g, steps)


def test_two_partitions_with_tile_offsets():
    """two partitions of a 48 x 48 mesh in one process (loopback halo exchange), C = 8: the edge and project kernels run over the
    boundary and the interior tiles with tile0 != 0.  A partition tiles its edges differently from the model, so the merged result
    is held to the float64 oracle alone: bound (a) per row, twice the model's own error globally."""
    from importlib import import_module
    halo = import_module("mgn_amd.halo")
    g = bc.reference_mesh(48, 48)
    stream = torch.cuda.current_stream().cuda_stream
    with Switches(C8):
        engs = []
        try:
            for k in range(2):
                p = engine_for(bc.CFG, rank=k, nranks=2, dtype="bf16")
                p.set_stream(stream)
                p.set_params(bc.params())
                p.set_graph(g.s, g.r, g.N, mesh_pos=g.pos)
                p.latents_import(g.v, g.e)
                engs.append(p)
            for p in engs:
                tb, nt = p.edge_boundary_tiles()
                ntn = (p.n_own + TILE - 1) // TILE
                ntb = (p.boundary_count() + TILE - 1) // TILE
                assert ntn > C8 and 0 < ntb < ntn                                # the pipe kernels; k_project_bf16_pipe at tile0 = ntb
                assert tb > 0 and nt - tb > 3 * C8                               # k_edge_bf16_pipe at tile0 = tb over the interior tiles
            mgn_amd.run_processor_staged(engs, halo.LoopbackExchange(engs, torch.device("cuda")), NSTEPS)
            torch.cuda.synchronize()
            fam = last_kernels()
            v, e = np.zeros((g.N, 128), np.float32), np.zeros((g.E, 128), np.float32)
            for p in engs:
                p.latents_export(v, e)
        finally:
            for p in engs:
                p.close()
    k = NSTEPS - 1
    print(f"two partitions: N={g.N} E={g.E}: families {fam}")
    assert fam == bc.PIPE, fam
    fails = []
    for i, (name, got) in enumerate((("v", v), ("e", e))):
        assert np.isfinite(got).all()
        to_orc, glob = rmax(row_rel(got, g.orc[k][i])), rel_l2(got, g.orc[k][i])
        ba, bg = 2.0 * g.model_err[k][i], 2.0 * g.model_err[k][2 + i]
        print(f"    two partitions step {k + 1} {name}: per row to the oracle {to_orc:.2e} (bound (a) {ba:.2e}), global {glob:.2e} (<= {bg:.2e}); "
              f"to the single partition's model {rmax(row_rel(got, g.m64[k][i])):.2e}")
        if not (to_orc <= ba and glob <= bg):
            fails.append((name, to_orc, ba, glob, bg))
    assert not fails, fails


def test_plain_weight_preload_above_16k_tiles():
    """16 x 1 024 + 1 edge tiles: copy_to_lds16 of k_edge_bf16_pipe takes the plain loop (a device-side constant that does not follow
    the test CU count); 16 353 nodes, one step, on the device's own CU count"""
    g = bc.reference(rows_of(512, 1), rows_of(16 * 1024 + 1, 31), "mfma", 1)
    old = set_renumber(0)
    eng = engine_for(bc.CFG, dtype="bf16")
    try:
        eng.set_params(bc.params())
        eng.set_graph(g.s, g.r, g.N)
        assert np.array_equal(eng.local_edges(), g.order)
        steps, fams = drive(eng, g, 1)
    finally:
        eng.close()
        set_renumber(old)
    print(f"plain preload: N={g.N} E={g.E}: families {fams}")
    assert fams == [bc.PIPE], fams
    assert_bounds("plain preload", g, steps)


@pytest.mark.parametrize("name", ["edge 40C+3", "edge 8C"])
def test_placement_invariance(name):
    """the same graph at C = 8 and C = 16: other blocks, other waves per tile range, the same bits (no atomics; a receiver's pieces
    are summed in edge order whatever the walk)"""
    g = bc.case_ref(name)
    outs = []
    for C in (8, 16):
        with Switches(C):
            eng = engine_for(bc.CFG, dtype="bf16")
            try:
                eng.set_params(bc.params())
                eng.set_graph(g.s, g.r, g.N)
                outs.append(eng.processor_steps(g.v, g.e, NSTEPS) + (last_kernels(),))
            finally:
                eng.close()
    assert outs[0][2] == outs[1][2] == bc.PIPE, (outs[0][2], outs[1][2])
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


def test_no_override_is_left():
    assert set_num_cus(0) == 0 and set_kernel_path(0) == 0
