"""The ring kernels' fragment prefetch at the tile counts where an early or a late fragment would be the wrong one.

`hs_layer_ring` (split.hip) reads the weight fragments of a chain step from the LDS window ring one or two steps ahead of the step's MFMAs.
A read that reaches a window before its store is behind a barrier, or a window whose buffer has been given to the next one, multiplies by
another step's weights: errors of order 1, not of order 1e-5.  Where that can happen depends on how many tiles a wave runs, because the
ring is re-primed at the tile top (`rs_first<0>`), wraps from the last chain of a tile into the first chain of the next, and runs on
padding tiles in the waves that have no tile left in the block's last round.  So the cases give the waves of `k_edge_ring_hs<8>` (family
16), `k_edge_ring_hs<4>` (17) and `k_node_ring_hs` (11) exactly one, two and three tiles, and two or three rounds of which the last is a
padding tile for most waves, with last tiles of 1, 31 and 32 rows.

Built like test_gpu_large_mesh_regimes.py, whose helpers it uses: test CU count 8, the ragged graph with hubs, two processor steps, the
float64 oracle on every row at ROW_TOL = 2e-5 (that file's derivation), the family codes asserted.  At C = 8 a launch of eight-wave blocks
has 64 waves and one of four-wave blocks 32 (one block per test CU).  The cases pass on the commit before the prefetch changed as well
(its library through MGN_LIB_PATH): they guard the ring's schedule, not one order of its reads."""
import pytest

from test_gpu_large_mesh_regimes import C8, NODE_DEFAULT, check, e_node_case, n_edge_case, rows_of

pytestmark = pytest.mark.gpu

# (tiles, rows of the last tile): eight-wave blocks run from 4 C + 1 to 8 C tiles and above 12 C, four-wave blocks up to 4 C and from
# 8 C + 1 to 12 C (kernels.hip: launch_edge_step)
EDGE8 = [(8 * C8, 32, "every wave one tile: the ring primed once, no wrap"),
         (16 * C8, 31, "every wave two tiles: the first wrap into a tile top"),
         (24 * C8, 32, "every wave three tiles"),
         (12 * C8 + 1, 1, "two rounds, the second a padding tile for 31 of 64 waves"),
         (16 * C8 + 1, 31, "three rounds, the third a padding tile for all waves but one")]
EDGE4 = [(4 * C8, 32, "every wave one tile"),
         (8 * C8 + 1, 1, "three rounds, the third a padding tile for all waves but one: the others ran two tiles"),
         (12 * C8, 31, "every wave three tiles")]
NODE = [(8 * C8, 32, "every wave one tile"),
        (16 * C8, 31, "every wave two tiles"),
        (24 * C8, 32, "every wave three tiles"),
        (16 * C8 + 1, 1, "three rounds, the third a padding tile for all waves but one")]


@pytest.mark.parametrize("T,tail,what", EDGE8, ids=[f"{t}x{r}" for t, r, _ in EDGE8])
def test_edge_ring_hs8_one_two_three_tiles_per_wave(T, tail, what):
    check(n_edge_case(C8), rows_of(T, tail), C8, 16, NODE_DEFAULT)


@pytest.mark.parametrize("T,tail,what", EDGE4, ids=[f"{t}x{r}" for t, r, _ in EDGE4])
def test_edge_ring_hs4_one_two_three_tiles_per_wave(T, tail, what):
    check(n_edge_case(C8), rows_of(T, tail), C8, 17, NODE_DEFAULT)


@pytest.mark.parametrize("T,tail,what", NODE, ids=[f"{t}x{r}" for t, r, _ in NODE])
def test_node_ring_hs_one_two_three_tiles_per_wave(T, tail, what):
    check(rows_of(T, tail), e_node_case(C8), C8, 17, NODE_DEFAULT)
