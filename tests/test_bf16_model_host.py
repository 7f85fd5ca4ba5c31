"""The bf16 rounding model of the oracle (mgn_oracle.processor_steps_bf16) on the CPU: that it is the oracle when nothing rounds, that its
rounding is the engine's, that it stays inside the stated bf16 band, and -- the reason it exists -- that the per-row bound
tests/test_gpu_bf16_regimes.py builds from it sees a wrong row.  numpy only; the graphs are the GPU file's (tests/bf16_cases.py).

Sensitivity.  Bound 3 of the GPU file is, per array and step, twice the largest per-row relative L2 between the model with float32 sums
and with float64 sums.  Every fault below is planted in step 1 of the model and must move its row by at least 1.5 x that bound:
the first, a middle and the last piece of every hub dropped (node 0's two pieces too), the two carry rows of a tile exchanged under a
run of an ordinary node that straddles two tiles, node n given the aggregate of node n + 1, the last edge row of the last tile not
computed, one e row stored without its residual.  Measured over the 17 case graphs (row error / bound 3, smallest and largest):

  fault (32-row tiles; the 16-row case graph in brackets)         row error / bound 3
  hub of 40 rows = 2 + 32 + 6: first / middle / last piece           2.0 .. 5.9 / 15.8 .. 62.8 / 4.0 .. 11.2   [4 pieces: 5.1 / 12.9 / 8.8]
  hub of 80 rows = 8 + 32 + 32 + 8                                    2.1 .. 6.0 / 3.4 .. 19.7 / 2.1 .. 7.7     [6 pieces: 6.1 / 7.4 / 7.8]
  hub of 108 rows = 12 + 32 + 32 + 32 (graphs from 1 500 edges)       1.9 .. 3.8 / 3.4 .. 19.7 / 3.5 .. 8.3
  hub of 144 rows = 24 + 32 + 32 + 32 + 24 (graphs from 1 500 edges)  2.4 .. 4.9 / 2.4 .. 6.1 / 1.8 .. 6.9
  node 0, 40 rows = 32 + 8                                            17.6 .. 57.6 / 4.8 .. 13.2                [16 + 16 + 8: 15.2 / 11.3 / 13.7]
  carry rows of a tile exchanged                                      41.6 .. 155
  aggregate of node n + 1                                             38.1 .. 167
  last edge row of the last tile not computed                         90 .. 689
  e row without its residual                                          97 .. 737
  (bound 3 after step 1 on these graphs: v 3.2e-3 .. 7.9e-3, e 1.0e-3 .. 7.0e-3; the smallest ratio is 1.8, 1.5 is required)

Runs of 70 = 3 + 32 + 32 + 3 and 100 = 4 + 32 + 32 + 32 rows gave 1.3 for their end pieces, a run of 170 = 16 + 4 x 32 + 26 rows 1.1 and
one of 184 = 28 + 4 x 32 + 28 rows 1.2: the hubs of tests/bf16_cases.py are as long as these conditions allow.
"""
import numpy as np
import pytest

import bf16_cases as bc
import mgn_oracle as orc

MARGIN = 1.5
TOL_BF16 = 3e-2         # tests/test_gpu_bf16.py: the stated band, relative L2 over a whole array after 15 steps


def ref_bits(x):
    """round to nearest even on the bit pattern, one value at a time: the upper 16 bits, plus one if the lower 16 are more than half a
    unit, or exactly half and the upper half is odd"""
    out = []
    for u in np.asarray(x, np.float32).view(np.uint32).tolist():
        lo, hi = u & 0xFFFF, u >> 16
        if lo > 0x8000 or (lo == 0x8000 and (hi & 1)):
            hi += 1
        out.append((hi << 16) & 0xFFFFFFFF)
    return np.array(out, np.uint32)


def test_round_bf16_is_the_engines_rounding():
    bits = [0x00000000, 0x80000000, 0x3F800000, 0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0x3F80FFFF, 0xBF808000, 0xBF818000,
            0x00000001, 0x00007FFF, 0x00008000, 0x00008001, 0x00018000, 0x007FFFFF, 0x80008000, 0x80018000, 0x807FFFFF,     # denormals
            0x00800000, 0x7F7F0000, 0x7F7E8000, 0xFF7E8000, 0x477FE000, 0x3EFFFFFF]
    x = np.array(bits, np.uint32).view(np.float32)
    got = orc.round_bf16(x)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), ref_bits(x))
    assert not (got.view(np.uint32) & 0xFFFF).any()
    rng = np.random.default_rng(0)
    y = np.concatenate([rng.standard_normal(20000).astype(np.float32) * np.float32(10.0) ** rng.integers(-30, 30, 20000).astype(np.float32),
                        rng.integers(0, 0x7F000000, 20000).astype(np.uint32).view(np.float32)])
    y = np.concatenate([y, -y])
    assert np.array_equal(orc.round_bf16(y).view(np.uint32), ref_bits(y))
    # float64 input is taken to float32 first (the kernels round fp32 values), idempotent, and at most half a bf16 unit away
    z = rng.standard_normal((7, 128))
    assert np.array_equal(orc.round_bf16(z), orc.round_bf16(z.astype(np.float32)))
    assert np.array_equal(orc.round_bf16(orc.round_bf16(z)), orc.round_bf16(z))
    assert (np.abs(orc.round_bf16(z) - z) <= np.abs(z) * 2.0 ** -8).all()


def test_pieces_are_one_receiver_inside_one_tile():
    r = np.array([5, 5, 5, 5, 5, 5, 7, 9, 9, 9, 2, 2], np.int32)
    order = np.argsort(r, kind="stable")                          # 2 2 | 5 5 || 5 5 5 5 || 7 9 9 9   (tiles of four)
    starts, pr = orc.edge_pieces(r, order, 4)
    assert starts.tolist() == [0, 2, 4, 8, 9] and pr.tolist() == [2, 5, 5, 7, 9]
    starts, pr = orc.edge_pieces(r, order, 2)
    assert starts.tolist() == [0, 2, 4, 6, 8, 9, 10] and pr.tolist() == [2, 5, 5, 5, 7, 9, 9]
    assert orc.edge_pieces(r[:0], order[:0])[0].size == 0


@pytest.mark.parametrize("two_sets", [False, True])
def test_without_rounding_the_model_is_the_oracle(two_sets):
    if two_sets:
        Tn, tn, T1, t1, T2, t2 = bc.TWO_SETS
        g = bc.reference_two_sets(bc.rows_of(Tn, tn), bc.rows_of(T1, t1), bc.rows_of(T2, t2))
        cfg, set2 = bc.CFG2, (g.e2, g.s2, g.r2, g.order2)
    else:
        g = bc.case_ref("handover node C+1")
        cfg, set2 = bc.CFG, None
    for tile_rows in (16, 32):
        got = orc.processor_steps_bf16(bc.params(cfg), cfg, g.v, g.e, g.s, g.r, bc.NSTEPS, g.order, tile_rows=tile_rows, mode="exact", set2=set2,
                                       all_steps=True)
        for k in range(bc.NSTEPS):
            for a, ref in zip(got[k], g.orc[k]):
                assert np.abs(a - ref).max() <= 1e-12 * np.abs(ref).max()
    # and the rounding modes are not the oracle: the model is a model of something
    assert bc.rel_l2(g.m64[0][0], g.orc[0][0]) > 1e-3


@pytest.mark.parametrize("name", list(bc.CASES))
def test_case_graphs_hold_what_they_are_built_for(name):
    """piece counts from the edge order, node 0, the receivers without an edge, the last tiles"""
    Tn, tn, Te, te, C, path, mode, codes = bc.CASES[name]
    g = bc.case_ref(name)
    assert g.N == bc.rows_of(Tn, tn) and g.E == bc.rows_of(Te, te) and tn in (1, 31, 32) and te in (1, 31, 32)
    assert np.array_equal(np.sort(g.order), np.arange(g.E)) and (np.diff(g.r[g.order]) >= 0).all()
    hp, starts, pr = bc.hub_pieces(g, bc.TILE)
    want = {rows: pieces for rows, _, pieces in bc.hubs_for(g.E)}
    assert len(hp) == len(want) >= 1
    for h, idx in hp.items():
        p0, rows = g.hubs[h]
        assert (g.r == h).sum() == rows and len(idx) == want[rows], (h, rows, len(idx))
    if g.E >= 1500:
        by_rows = {rows: (p0, h) for h, (p0, rows) in g.hubs.items()}
        assert (by_rows[108][0] + 108) % bc.TILE == 0                                     # ends exactly on a tile boundary
        assert [len(hp[by_rows[n][1]]) for n in (40, 80, 108, 144)] == [3, 4, 4, 5]
    p0, _ = next((p, n) for h, (p, n) in g.hubs.items() if n == 40)
    sizes = np.diff(np.append(starts, g.E))
    first = np.searchsorted(starts, p0)
    assert sizes[first:first + 3].tolist() == [2, 32, 6]                                  # a 2-edge piece, a whole tile of one receiver
    assert (g.r == 0).sum() == 40 and (g.s == 0).sum() >= 40 and (g.r[g.order][:40] == 0).all()
    recv = np.bincount(g.r, minlength=g.N) > 0
    last_tile0 = (g.N - 1) // bc.TILE * bc.TILE
    assert not recv[last_tile0 - bc.TILE:].any() and not recv[g.N - g.N // 8:].any()   # a whole node tile and the last node
    assert np.bincount(g.r).max() <= 400


BAND_CASES = [n for n in bc.CASES if not n.startswith("walk")] + ["walk 192C+1"]


@pytest.mark.parametrize("name", BAND_CASES)
def test_model_is_inside_the_stated_band_after_15_steps(name):
    """(of the five walk graphs one: the others are the same construction with 9 or 2 tiles fewer of 1 537, or at twice the size, and
    15 steps of the two references on each take 13 to 40 s)"""
    Tn, tn, Te, te, C, path, mode, codes = bc.CASES[name]
    g = bc.case_ref(name)
    cfg = dict(bc.CFG, mps=15)
    ps = bc.params(cfg)
    rv, re = orc.processor_steps(ps, cfg, g.v, g.e, g.s, g.r, 15)
    mv, me = orc.processor_steps_bf16(ps, cfg, g.v, g.e, g.s, g.r, 15, g.order, tile_rows=g.tile_rows, mode=mode)
    band = (bc.rel_l2(mv, rv), bc.rel_l2(me, re))
    print(f"{name}: model against the oracle after 15 steps, relative L2: v {band[0]:.2e} e {band[1]:.2e}; "
          f"after 1 and 2 steps: {g.model_err[0][2]:.2e} {g.model_err[0][3]:.2e}, {g.model_err[1][2]:.2e} {g.model_err[1][3]:.2e}")
    assert max(band) <= TOL_BF16, band
    assert max(band) >= 1e-3                # bf16 arithmetic, not the oracle again


def straddling_pair(g, starts, pr, used):
    """pieces (p, p + 1) of an ordinary node whose run lies in two consecutive tiles, and what the exchanged carry rows of those tiles
    hold instead: the first piece of the first tile if it continues a run from the tile before, the last piece of the second tile if
    its run goes on into the next one -- else a row no kernel of this step wrote (zero)"""
    tile = starts // g.tile_rows
    cnt = np.bincount(pr, minlength=g.N)
    two = [p for p in range(1, len(pr) - 2) if pr[p] not in used and cnt[pr[p]] == 2 and pr[p + 1] == pr[p]]
    more = [p for p in range(1, len(pr) - 2) if pr[p] not in used and pr[p + 1] == pr[p] and pr[p - 1] != pr[p]]      # (dense graphs: the first two pieces of a longer run)
    for p in two + more:
        n = pr[p]
        assert tile[p + 1] == tile[p] + 1
        q0 = int(np.searchsorted(tile, tile[p], "left"))
        q1 = int(np.searchsorted(tile, tile[p + 1], "right")) - 1
        src0 = q0 if (q0 > 0 and q0 != p and pr[q0] == pr[q0 - 1]) else -1
        src1 = q1 if (q1 + 1 < len(pr) and q1 != p + 1 and pr[q1] == pr[q1 + 1]) else -1
        return int(n), {p: src0, p + 1: src1}
    raise AssertionError("no ordinary node with a run over two tiles")


def sensitivity(g, cfg=bc.CFG):
    """[(fault, array, row, row error / bound 3)] of one case graph"""
    hp, starts, pr = bc.hub_pieces(g)
    zero_pieces = np.nonzero(pr == 0)[0]
    runs = dict(hp)
    runs[0] = zero_pieces
    used = set(runs)
    n_sw, swap = straddling_pair(g, starts, pr, used)
    used.add(n_sw)
    cnt = np.bincount(g.r, minlength=g.N)
    n_ag = next(n for n in range(1, g.N - 1) if n not in used and n + 1 not in used and cnt[n] > 0 and cnt[n + 1] > 0)
    row_last = g.E - 1                                              # engine row: the last edge row of the last tile
    e_nores = int(g.order[g.E // 3])
    assert e_nores != g.order[row_last] and g.r[g.order[row_last]] not in used | {n_ag}
    b3v, b3e = 2.0 * g.spread[0][0], 2.0 * g.spread[0][1]
    base_v, base_e = g.m64[0][0], g.m64[0][1]
    out = []
    for which in ("first", "middle", "last"):
        drop = {int(idx[{"first": 0, "middle": len(idx) // 2, "last": -1}[which]]): -1 for idx in runs.values()}
        fault = dict(step=0, piece_src=dict(drop))
        if which == "first":
            fault["piece_src"].update(swap)
            fault.update(agg_from={n_ag: n_ag + 1}, drop_row=row_last, no_residual=e_nores)
        v1, e1 = orc.processor_steps_bf16(bc.params(cfg), cfg, g.v, g.e, g.s, g.r, 1, g.order, tile_rows=g.tile_rows, mode=g.mode, fault=fault)
        dv, de = bc.row_rel(v1, base_v), bc.row_rel(e1, base_e)
        for h, idx in runs.items():
            p = int(idx[{"first": 0, "middle": len(idx) // 2, "last": -1}[which]])
            rows = int(np.append(starts, g.E)[p + 1] - starts[p])
            out.append((f"{which} piece ({rows} rows) of the {len(idx)} pieces of node {h}", "v", h, dv[h] / b3v))
        if which == "first":
            out.append(("carry rows of a tile exchanged", "v", n_sw, dv[n_sw] / b3v))
            out.append(("aggregate of node n + 1", "v", n_ag, dv[n_ag] / b3v))
            out.append(("last edge row not computed", "e", int(g.order[row_last]), de[g.order[row_last]] / b3e))
            out.append(("e row without its residual", "e", e_nores, de[e_nores] / b3e))
            # nothing but the planted rows moved: the faults of one run do not touch each other
            touched = set(runs) | {n_sw, n_ag, int(g.r[g.order[row_last]])}
            assert set(np.nonzero(dv > 0)[0].tolist()) <= touched
            assert set(np.nonzero(de > 0)[0].tolist()) == {int(g.order[row_last]), e_nores}
    return out


@pytest.mark.parametrize("name", list(bc.CASES))
def test_bound_3_sees_every_planted_fault(name):
    g = bc.case_ref(name)
    res = sensitivity(g)
    print(f"{name} (bound 3 after step 1: v {2 * g.spread[0][0]:.2e} e {2 * g.spread[0][1]:.2e})")
    for what, arr, row, ratio in res:
        print(f"    {what}: {arr} row {row} moved by {ratio:.1f} x bound 3")
    low = [(what, ratio) for what, arr, row, ratio in res if not ratio >= MARGIN]
    assert not low, low
