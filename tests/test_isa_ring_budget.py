"""What hipcc makes of the ring kernels' between-chain code (host only: split.hip is compiled to gfx950 assembly, nothing runs).

Every vector instruction outside an MFMA chain is paid in full by both waves of a SIMD (docs/experiments.md), and the compiler has twice
added work there that the algorithm does not ask for: a canonicalising `v_max_f32 v, x, x` (or `|x|, |x|`) ahead of every fmaxf whose
input comes from a load or an MFMA, and a ds_bpermute_b32 + LDS wait for every exchange between the lane halves.  h2_rowmax is budgeted
at 32 v_max3_f32 per call -- three calls per edge tile, five per node tile -- and the exchanges at one v_permlane32_swap_b32 / DPP move
each.  This test keeps the object at that budget, and the kernels at the scratch they had."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)

pytestmark = pytest.mark.skipif(HIPCC is None, reason="hipcc not found")

EDGE, NODE = "k_edge_ring_hsILi8", "k_node_ring_hs"
NODE_SCRATCH_BEFORE = 20        # bytes: .private_segment_fixed_size of k_node_ring_hs in the object of the commit before h2_rowmax became instructions


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("isa") / "split.s")
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "include"), "-S", "--cuda-device-only",
                           os.path.join(ROOT, "meshgraphnets.jl_amd", "csrc", "split.hip"), "-o", out], stderr=subprocess.DEVNULL)
    return open(out).read().splitlines()


def body(asm, key):
    import isa_mix
    s, e = isa_mix.kernel_body(asm, key)
    return isa_mix.instructions(asm, s, e)


@pytest.mark.parametrize("key", [EDGE, NODE])
def test_no_canonicalising_maxima(asm, key):
    same = []
    for n, m, ops in body(asm, key):
        if re.match(r"v_max_f32(_e32|_e64)?$", m):
            o = [x.strip() for x in ops.split(",")]
            if len(o) == 3 and o[1] == o[2]:
                same.append((n, m, ops))
    assert not same, same[:4]


@pytest.mark.parametrize("key", [EDGE, NODE])
def test_no_lds_round_trip_for_a_lane_exchange_in_the_tile_loop(asm, key):
    import isa_mix
    loop = isa_mix.tile_loop(body(asm, key))
    assert sum(1 for _, m, _ in loop if m.startswith("v_mfma")) >= 288          # it is the tile loop: three chains of 96 MFMAs at least
    assert not [x for x in loop if x[1].startswith("ds_bpermute")]
    assert [x for x in loop if x[1].startswith("v_permlane32_swap")]


@pytest.mark.parametrize("key,calls", [(EDGE, 3), (NODE, 5)])
def test_row_maxima_fold_two_values_per_instruction(asm, key, calls):
    n = sum(1 for _, m, _ in body(asm, key) if m.startswith("v_max3_f32"))
    assert n >= 32 * calls, n


def test_scratch_did_not_grow(asm):
    import isa_mix
    assert isa_mix.resources(asm, EDGE)["private_segment_fixed_size"] == 0
    assert isa_mix.resources(asm, NODE)["private_segment_fixed_size"] <= NODE_SCRATCH_BEFORE
