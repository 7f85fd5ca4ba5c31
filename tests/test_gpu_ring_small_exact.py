"""The two ring kernels of the processor step at the smallest meshes that select them, against the float64 oracle and against themselves.

With the test CU count (mgn_debug_num_cus(8); test_gpu_large_mesh_regimes.py) 17 edge tiles run k_edge_ring_hs<4> (family 17) and 33 run
k_edge_ring_hs<8> (16); 17 node tiles run k_node_ring_hs (11) on every step that projects the next one's P / Q.  Their row maxima
(h2_rowmax) and LayerNorm sums meet across the two lane halves of a wave; a wrong exchange would be deterministic, so each case is held
to the oracle at the fp32 tolerances AND, run a second time from the same inputs, to its own bits.  Both meshes end in a partly filled
tile (1 and 31 rows): the padding rows pass through the same maxima.  The graphs, latents and oracle results are the regime module's
(built once per session, read-only)."""
import numpy as np
import pytest
import torch  # noqa: F401  (before the engine's first HIP call)

import test_gpu_large_mesh_regimes as lm

pytestmark = pytest.mark.gpu

C = lm.C8
NODE_TILES = 2 * C + 1                                            # above two tiles per CU: the split-path node kernels start here


@pytest.mark.parametrize("edge_tiles,tail,edge_code", [(2 * C + 1, 1, 17), (4 * C + 1, 31, 16)], ids=["ring_hs4", "ring_hs8"])
def test_smallest_ring_meshes_meet_the_oracle_twice_with_the_same_bits(edge_tiles, tail, edge_code):
    N, E = lm.rows_of(NODE_TILES, 1), lm.rows_of(edge_tiles, tail)
    assert N % lm.TILE == 1 and E % lm.TILE == tail % lm.TILE     # last node tile: one row; last edge tile: 1 / 31 rows
    # families asserted step by step (mgn_debug_last_edge_kernel / _node_kernel), two processor steps against float64 at TOL_15, per row
    # at ROW_TOL, and no worse than twice the fp32-MFMA kernels
    v1, e1, _ = lm.check(N, E, C, edge_code, lm.NODE_DEFAULT)
    v2, e2, fams, _ = lm.run(N, E, C)
    assert fams == [(edge_code, n) for n in lm.NODE_DEFAULT], fams
    assert np.array_equal(v1, v2) and np.array_equal(e1, e2)
