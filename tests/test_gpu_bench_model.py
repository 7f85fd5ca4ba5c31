"""bench.py's `secondary.scaling_model` (2 / 4 / 8 GPUs predicted from one: the real partition's shares through the staged schedule) on a
small mesh: it has to run on a one-GPU box -- the driver's bench run is not the place to find out that it does not.  And the plain bench
line (no --full) with the outputs it dumps."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mgn_amd  # noqa: E402

pytestmark = pytest.mark.gpu


def test_scaling_model_runs_and_adds_up():
    import torch
    import bench
    pos, s, r = mgn_amd.synth.mesh_1m(1234, 180, 180)
    N, E = pos.shape[0], int(s.size)
    ps = bench.glorot_params()

    def sync():
        torch.cuda.synchronize()

    m = bench.scaling_model(ps, pos, s, r, N, E, 1e-4, 0, sync)
    for P in (2, 4, 8):
        d = m[f"{P}_gpus"]
        assert abs(d["n_own"] - N / P) <= 1 and d["n_halo"] > 0 and d["send_rows"] > 0
        assert d["edge_tiles_boundary"] > 0 and d["edge_tiles_interior"] > d["edge_tiles_boundary"]
        assert np.isfinite(d["share_ms_per_step_staged"]) and d["share_ms_per_step_staged"] > 0
        assert d["predicted_ms_per_step"] >= d["share_ms_per_step_staged"]
        assert d["predicted_edges_per_s"] == pytest.approx(E / (d["predicted_ms_per_step"] * 1e-3))
        assert 0 < d["pack_us"] < 1e4 and 0 < d["unpack_us"] < 1e4
    assert m["8_gpus"]["share_ms_per_step_staged"] < m["2_gpus"]["share_ms_per_step_staged"]


def _bench_line(*args):
    import json
    import subprocess
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args], capture_output=True, text=True,
                         timeout=600, cwd=ROOT)
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert res.returncode == 0 and len(lines) == 1, res.stdout[-1500:] + res.stderr[-3000:]
    return json.loads(lines[0])


def test_plain_bench_line_and_dumped_outputs(tmp_path):
    """A plain run (no --full) prints the headline alone over exactly --steps timed steps, and --dump-outputs writes what the last
    timed step left: the same bits from two runs with the same arguments, and the same bits as the engine gives after W + K passes
    from the bench's inputs (seeded parameters, mesh and latents)."""
    import bench
    nx, steps, warmup = 100, 3, 2
    args = ["--steps", str(steps), "--warmup", str(warmup), "--nx", str(nx)]
    d = _bench_line(*args, "--dump-outputs", str(tmp_path / "a"))
    pos, s, r = mgn_amd.synth.mesh_1m(1234, nx, nx)
    N, E = pos.shape[0], int(s.size)
    assert d["metric"] == "processor-step edges/s" and d["unit"] == "edges/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["steps"] == steps and d["warmup"] == warmup and d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(E * bench.MPS * 1e3 / d["ms_per_step"], rel=1e-9)
    assert not {"median", "roofline", "latents_finite", "secondary", "cpu_baseline"} & set(d)
    v = np.load(tmp_path / "a" / "node_latents.npy")
    e = np.load(tmp_path / "a" / "edge_latents.npy")
    assert v.dtype == e.dtype == np.float32 and v.shape == (N, bench.L) and e.shape == (bench.DUMP_ROWS, bench.L)
    assert N <= bench.DUMP_ROWS < E                                      # all node rows, a sample of the edge rows
    assert v.nbytes + e.nbytes <= 64 << 20 and np.isfinite(v).all() and np.isfinite(e).all()

    _bench_line(*args, "--dump-outputs", str(tmp_path / "b"))
    assert np.array_equal(np.load(tmp_path / "b" / "node_latents.npy"), v)
    assert np.array_equal(np.load(tmp_path / "b" / "edge_latents.npy"), e)

    eng = mgn_amd.Engine(bench.FN, bench.FE, bench.O, bench.L, 2, bench.MPS, device=0)
    try:
        eng.set_params(bench.glorot_params())
        eng.set_graph(s, r, N, mesh_pos=pos)
        eng.latents_randn(1234)
        for _ in range(warmup + steps):
            eng.processor_steps_dev(bench.MPS)
        rv, re_ = eng.latents_export()
    finally:
        eng.close()
    assert np.array_equal(rv[bench.dump_rows(N, 1)], v) and np.array_equal(re_[bench.dump_rows(E, 2)], e)
