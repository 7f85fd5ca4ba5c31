"""The three stage MLPs around the processor -- node encoder (+ the step-0 P / Q projection), edge encoder, decoder -- each on its
own against the float64 oracle, in every kernel family of launch_enc_node / launch_enc_edge / launch_decode (kernels.hip).
Run on the MI355X box with `-m gpu`.

Which family a case reaches is size arithmetic at set_num_cus(8) (no code records the family of these launches); N nodes are
ceil(N / 32) node tiles, E edges ceil(E / 32) edge tiles:

  cooperative, fenced    path 0, N = 70 (3 tiles), E = 200 (7): cooperative up to 8 x 8 = 64 node and 16 x 8 = 128 edge tiles,
                         pinned weight rings up to 4 x 8 = 32 tiles
  cooperative, unfenced  path 0, N = 1061 (34 tiles), E = 1287 (41): in the cooperative range, above 32 tiles
  resident, 8 waves      path 0, N = 2083 (66 tiles > 64), E = 4137 (130 > 128): above the cooperative range and above the 4 x 8
                         tiles of a streaming launch; 8 blocks of 8 waves, so waves walk a second tile, and the last tile is
                         ragged (2083 = 65 x 32 + 3, 4137 = 129 x 32 + 9)
  streaming (NRES = 0)   path 2, N = 70, E = 200
  resident, 1 wave       path 1, N = 70, E = 200: at most 8 tiles, one-wave blocks
  GEN                    path 4 at hidden_layers 2, path 0 at hidden_layers 1 and 3; L = 32, 64, 128
  L = 64, L = 32         path 0, hidden_layers 2: the resident instantiations with every chunk of the stage in LDS

The L = 128 rows with hidden_layers 2 run on the chunks' two fp16 pieces (set_split_f16(1)) and on the fp32 fragments (0).

Bound: rel_max <= TOL_STEP for every array.  Largest rel_max / TOL_STEP per family on the parent of the commit that added this
file (encode v, encode e, step-0 edge update, decode):
  family           encode v  encode e  step-0 e  decode
  coop_fenced      0.019     0.020     0.019     0.012
  coop_unfenced    0.017     0.020     0.021     0.017
  resident8        0.021     0.021     0.023     0.013
  streaming        0.019     0.020     0.029     0.012
  resident1        0.019     0.020     0.029     0.012
  gen              0.019     0.023     0.029     0.015
  tuned (L 64/32)  0.010     0.018     0.023     0.013
No family comes near the bound on the parent; the commit itself left every one of these arrays bit-equal.
"""
import numpy as np
import pytest
import torch   # noqa: F401  before the first HIP call of libmgn_hip: torch must initialise its own runtime first

import mgn_amd
import mgn_oracle as orc
from mgn_amd import synth
from util import TOL_STEP, rel_max, set_kernel_path, set_num_cus, set_renumber, set_split_f16

pytestmark = pytest.mark.gpu

SMALL, MID, BIG = (70, 200), (1061, 1287), (2083, 4137)
# (family, (N, E), L, hidden_layers, kernel path, split_f16)
CASES = [(fam, ne, 128, 2, path, f16)
         for fam, ne, path in (("coop_fenced", SMALL, 0), ("coop_unfenced", MID, 0), ("resident8", BIG, 0),
                               ("streaming", SMALL, 2), ("resident1", SMALL, 1))
         for f16 in (1, 0)]
CASES += [("gen", SMALL, L, h, 4 if h == 2 else 0, 1) for L in (32, 64, 128) for h in (2, 1, 3)]
CASES += [("tuned", SMALL, L, 2, 0, 1) for L in (64, 32)]


def case_id(c):
    fam, (N, _), L, h, path, f16 = c
    return f"{fam}-N{N}-L{L}-h{h}-path{path}-{'f16' if f16 else 'f32'}"


@pytest.fixture(params=CASES, ids=case_id)
def stage(request):
    """An engine of the case with the switches set before it is created, and the float64 model beside it."""
    fam, (N, E), L, h, path, f16 = request.param
    old = set_num_cus(8), set_renumber(0), set_kernel_path(path), set_split_f16(f16)
    assert old[0] >= 0
    try:
        cfg = dict(Fn=9, Fe=3, O=2, L=L, hidden_layers=h, mps=1)
        ps = orc.init_params(9, 3, 2, L, h, 1, seed=1234, ln_jitter=0.1)
        s, r = synth.random_graph(N, E, seed=N)
        rng = np.random.default_rng(N + L + h)
        nf = rng.standard_normal((N, 9)).astype(np.float32)
        ef = rng.standard_normal((E, 3)).astype(np.float32)
        eng = mgn_amd.Engine(9, 3, 2, L, h, 1)
        eng.set_params(ps)
        eng.set_graph(s, r, N)
        yield dict(eng=eng, P=orc._unpack(ps, cfg, np.float64), h=h, L=L, s=s, r=r, nf=nf, ef=ef, rng=rng)
    finally:
        set_split_f16(old[3])
        set_kernel_path(old[2])
        set_renumber(old[1])
        set_num_cus(old[0])


def test_encode_padding_and_step0_projection(stage):
    eng, P, h = stage["eng"], stage["P"], stage["h"]
    rv, re = orc.encode(P, stage["nf"].astype(np.float64), stage["ef"].astype(np.float64), h)
    eng.fwd_upload(stage["nf"], stage["ef"])
    eng.fwd_encode()
    v, e = eng.latents_export()
    chk = eng.latents_checksum()
    print("encode", rel_max(v, rv) / TOL_STEP, rel_max(e, re) / TOL_STEP)
    assert rel_max(v, rv) <= TOL_STEP, rel_max(v, rv)
    assert rel_max(e, re) <= TOL_STEP, rel_max(e, re)
    # the padding rows of the tile-major arrays are zero: the device's sums over whole tiles are the sums of the exported rows
    v64, e64 = v.astype(np.float64), e.astype(np.float64)
    for got, want in ((chk["sum_v"], v64.sum()), (chk["sumsq_v"], (v64 * v64).sum()),
                      (chk["sum_e"], e64.sum()), (chk["sumsq_e"], (e64 * e64).sum())):
        assert np.isclose(got, want, rtol=1e-9, atol=0.0), (got, want)
    # P, Q of step 0 as the first edge step reads them: e + MLP_e([v[s]; v[r]; e])
    eng.proc_edge(0)
    e1 = eng.edge_latents_export(0)
    re1 = re + orc.mlp(np.concatenate([rv[stage["s"]], rv[stage["r"]], re], 1), P["proc0_edge"], h)
    print("step0_edge", rel_max(e1, re1) / TOL_STEP)
    assert rel_max(e1, re1) <= TOL_STEP, rel_max(e1, re1)


def test_decode(stage):
    eng, P, h, L = stage["eng"], stage["P"], stage["h"], stage["L"]
    v = stage["rng"].standard_normal((eng.N, L)).astype(np.float32)
    e = stage["rng"].standard_normal((eng.E, L)).astype(np.float32)
    eng.latents_import(v, e)
    eng.fwd_decode()
    out = eng.fwd_download()
    ref = orc.decode(P, v.astype(np.float64), h)
    print("decode", rel_max(out, ref) / TOL_STEP)
    assert rel_max(out, ref) <= TOL_STEP, rel_max(out, ref)
