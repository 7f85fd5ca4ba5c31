"""Where hipcc puts the ring kernels' fragment reads and their waits (host only: split.hip is compiled to gfx950 assembly, nothing runs).

hs_layer_ring asks for the weight fragments of step it + D at the top of step it and waits, with counted lgkmcnt values, for one
fragment in front of the MFMA that takes it.  The source order alone does not give that: left alone hipcc moves a step's first MFMA
above the reads and drains the LDS queue in front of every step (docs/experiments.md).  This test reads the emitted order with
tools/isa_chain.py: in every chain of the tile loop the only drains are the window barriers' (eight windows: seven barriers inside the
chain), and every fragment read is issued at least a whole step -- three MFMAs -- ahead of the wait that covers it."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)

pytestmark = pytest.mark.skipif(HIPCC is None, reason="hipcc not found")

WINDOWS_PER_CHAIN = 8           # split.hip: RsT::WPL


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("isa") / "split.s")
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "include"), "-S", "--cuda-device-only",
                           os.path.join(ROOT, "meshgraphnets.jl_amd", "csrc", "split.hip"), "-o", out], stderr=subprocess.DEVNULL)
    return open(out).read().splitlines()


@pytest.mark.parametrize("key,nchains", [("k_edge_ring_hsILi8", 3), ("k_edge_ring_hsILi4", 3), ("k_node_ring_hs", 6)])
def test_fragment_reads_run_a_step_ahead_of_counted_waits(asm, key, nchains):
    import isa_chain
    import isa_mix
    s, e = isa_mix.kernel_body(asm, key)
    ins = [x for x in isa_mix.tile_loop(isa_mix.instructions(asm, s, e)) if x[1] != "label" and isa_mix.classify(x[1])]
    spans = isa_chain.chains(ins)
    assert len(spans) == nchains, spans
    for c, (a, b) in enumerate(spans):
        forms, dist, _ = isa_chain.chain_report(ins, a, b)
        assert sum(1 for x in ins[a:b + 1] if isa_mix.classify(x[1]) == "mfma") == 96
        drains = sum(n for f, n in forms.items() if isa_chain.lgkm(f) == 0)
        counted = sum(n for f, n in forms.items() if (isa_chain.lgkm(f) or 0) > 0)
        print(key, "chain", c, "drains", drains, "counted", counted, "MFMAs between read and wait: min", min(d[0] for d in dist))
        assert drains <= WINDOWS_PER_CHAIN - 1, (c, forms)
        assert counted >= 32, (c, forms)                    # a counted wait per step at least
        assert len(dist) >= 56, (c, len(dist))              # the chain's fragment reads (62 less the few a chain's ends move out of it)
        assert min(d[0] for d in dist) >= 3, (c, sorted(dist)[:4])
