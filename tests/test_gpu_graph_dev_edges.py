"""The device graph prologue (csrc/graph_dev.hip: k_one_hot, k_edge_features, the uniform-grid world-edge search, the triangle-to-edge
keys; driven by mgn_set_static_mesh, mgn_world_edges_dev and mgn_triangles_to_edges_dev) at the edges of its input space, against
brute-force references: the dense float64 search, the float64 oracle, and the host C++ as a second witness.  The cases and references
are tests/graph_prologue_cases.py; tests/test_graph_prologue_host.py holds the same table against the host side where no GPU is needed.

Integer results are compared as arrays.  The static inputs are compared through mgn_ode_step BIT FOR BIT: on the dyadic lattices of the
case table the float64 one-hot rows and edge features round to float32 without error (up to the square root, which is correctly
rounded on both sides), so mgn_set_static with the oracle's arrays and mgn_set_static_mesh feed identical values to identical kernels --
one wrong one-hot column of a rare type or one wrong sign in a feature column changes bits.  (It does hold bit for bit on the MI355X,
f32 and bf16, plain and renumbered handles: neither the contraction of n2 += v * v, exact here either way, nor sqrtf shows.)

45 tests, 4 s of wall time on an MI355X (the slowest, 1 s, is the float64 oracle on the 117 306 world edges of the one-cell lattice).

Scratch mutations of the library, tried on a copy, one at a time, each wrong in values only (every access stays in bounds); what fails:
  * k_world_search, `d2 < r2` -> `d2 <= r2`: test_world_edges_dev_every_case_on_one_handle[1], [2] and [3] (the lattice distances that
    equal the radius); nothing else.
  * k_one_hot without `- type_min`: every case with type_min != 0 (1..7, -2..4 twice, the depth-1 case at type 5) of
    test_set_static_mesh_bit_equals_set_static, ..._on_scattered_labels and ..._meets_the_oracle_rhs, 20 tests; none with type_min = 0.
  * k_edge_features with sender and receiver swapped: every case of the three set_static_mesh tests, the refusal test and
    test_world_edges_dev_feed_the_model[lattice 3-D r=10], 37 tests; NOT the coincident-point case of that test (400 of its 400-odd
    feature rows are zeros, the rest meets TOL_15 with the signs flipped) -- the bit comparisons are what holds the sign.
  * mgn_set_static_mesh passing l2g = nullptr on a renumbered handle: all 14 of test_set_static_mesh_on_scattered_labels, nothing else.
  * fenc without the sign fold (the host's fdec unchanged): NO new test fails, and none can by values: the decoded bounding box is wrong
    wherever a coordinate is negative (a NaN corner with -0.0), but the box only places the grid.  The cell size stays >= the radius and
    cell_of clamps monotonically, so neighbours stay in neighbouring cells and the search returns the same edges from a worse grid.  (The
    grid sizes such a box yields were worked out on the host for every case here before the mutant ran: 1 <= cells <= the allocated cap.)
"""
import ctypes as C

import numpy as np
import pytest
import torch

import graph_prologue_cases as gc
import mgn_amd
import mgn_oracle as orc
from test_gpu_two_edge_sets import TOL_15, cfg2, engine2, params2
from util import cfg_dict, engine_for, make_params, rel_max, renumbered, set_renumber

pytestmark = pytest.mark.gpu


def _key(s, r):
    return s.astype(np.int64) * (1 << 20) + r


def _assert_world_edges(eng, s0, r0, what):
    """the installed set 1 against the dense search (s0, r0), in the order include/mgn_hip.h promises: receiver-major with ascending senders
    in the ENGINE's node numbering -- the caller's, and then the dense search's arrays entry for entry, unless mgn_set_graph renumbered"""
    sd, rd = eng.edge_set_export(1)
    assert eng.edge_set_info(1)[0] == s0.size == sd.size, what
    if not renumbered(eng):
        assert np.array_equal(sd, s0) and np.array_equal(rd, r0), what
        return
    own = eng.owned_nodes()
    assert np.array_equal(np.sort(own), np.arange(own.size)), what
    inv = np.argsort(own)                                            # caller's id -> engine id
    assert np.array_equal(np.sort(_key(sd, rd)), np.sort(_key(s0, r0))), what
    assert np.all(np.diff(_key(inv[rd], inv[sd])) > 0), what


# ---- world edges -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_world_edges_dev_every_case_on_one_handle(dim):
    """every case of one dim in sequence on ONE handle: E2 goes large -> 0 -> large and the work buffers are reused; the graph is set
    again whenever N or the mesh list changes"""
    eng = mgn_amd.Engine(12, 7, 3, 128, 2, 3, Fe2=dim + 1)
    graph = None
    sizes = []
    for name, (pos, rad, ms, mr) in gc.WORLD_CASES.items():
        if pos.shape[1] != dim:
            continue
        if graph is None or graph[0] != pos.shape[0] or not np.array_equal(graph[1], ms) or not np.array_equal(graph[2], mr):
            eng.set_graph(ms, mr, pos.shape[0])
            graph = (pos.shape[0], ms, mr)
        s0, r0 = gc.world_reference(name)
        sh, rh = mgn_amd.world_edges_native(pos, rad, ms, mr)
        n = eng.world_edges_dev(1, pos, rad)
        assert n == s0.size and np.array_equal(sh, s0) and np.array_equal(rh, r0), name
        _assert_world_edges(eng, s0, r0, name)
        # (the one case with a mesh list gives mgn_set_graph a radius graph under random labels: it renumbers, and the order is the engine's)
        assert renumbered(eng) == (ms.size > 0), name
        sizes.append(n)
    assert len(sizes) >= 7 and 0 in sizes[1:-1] and max(sizes) > 1000
    if dim == 3:
        assert tuple(sizes[:6]) == gc.LATTICE3_COUNTS
    eng.close()


def test_world_edges_dev_takes_device_positions():
    """include/mgn_hip.h allows device pointers: the positions of a case in a torch device tensor, through the C ABI directly.  The case
    with a mesh list, here on a handle that keeps the caller's numbering: the dense search's arrays entry for entry."""
    name = "mesh list: one-way, duplicates, self loops"
    pos, rad, ms, mr = gc.WORLD_CASES[name]
    eng = mgn_amd.Engine(12, 7, 3, 128, 2, 3, Fe2=3)
    old = set_renumber(0)
    try:
        eng.set_graph(ms, mr, pos.shape[0])
    finally:
        set_renumber(old)
    assert not renumbered(eng)
    t = torch.from_numpy(pos.copy()).cuda()
    torch.cuda.synchronize()
    n = C.c_int64()
    assert eng.lib.mgn_world_edges_dev(eng.h, 1, t.data_ptr(), 2, C.c_float(rad), C.byref(n)) == 0
    s0, r0 = gc.world_reference(name)
    assert n.value == s0.size
    _assert_world_edges(eng, s0, r0, name)
    assert np.array_equal(t.cpu().numpy(), pos)
    eng.close()


@pytest.mark.parametrize("name", ["lattice 3-D r=10", "coincident r=0.05", "lattice 3-D r=0.001"])
def test_world_edges_dev_feed_the_model(name):
    """device-searched, device-featured world edges against the float64 oracle on the dense search's edges: hub receivers with 342 senders
    each and E2 no multiple of 32; feature rows of zeros between coincident points; no world edge at all"""
    pos, rad, ms, mr = gc.WORLD_CASES[name]
    s2, r2 = gc.world_reference(name)
    N = pos.shape[0]
    assert {"lattice 3-D r=10": s2.size % 32 != 0 and np.bincount(r2).min() == 342,
            "coincident r=0.05": (np.abs(gc.world_features(pos, s2, r2)).max(1) == 0).sum() == 400, "lattice 3-D r=0.001": s2.size == 0}[name]
    cfg = cfg2(128, 2)
    ps = params2(cfg)
    rng = np.random.default_rng(N + s2.size)
    nf = rng.standard_normal((N, 12)).astype(np.float32)
    ef = rng.standard_normal((ms.size, 7)).astype(np.float32)
    eng = engine2(cfg)
    eng.set_params(ps)
    eng.set_graph(ms, mr, N)
    assert eng.world_edges_dev(1, pos, rad) == s2.size
    out = eng.forward(nf, ef)
    ref = orc.forward(ps, cfg, nf, ef, ms, mr, set2=(gc.world_features(pos, s2, r2), s2, r2))
    print(f"{name}: E2 = {s2.size}, rel_max = {rel_max(out, ref):.3e}")
    assert rel_max(out, ref) <= TOL_15
    eng.close()


def test_world_edges_dev_on_a_renumbered_handle():
    """scattered node labels: the same SET as the dense search in the caller's ids, and -- what the engine really promises about the order,
    include/mgn_hip.h -- receiver-major with ascending senders in the ENGINE's numbering (the inverse of mgn_owned_nodes)"""
    pos, rad, ms, mr = gc.renumbered_world_case()
    N = pos.shape[0]
    s0, r0 = gc.dense_world_edges(pos, rad, ms, mr)
    sh, rh = mgn_amd.world_edges_native(pos, rad, ms, mr)
    assert s0.size > 1000 and np.array_equal(sh, s0) and np.array_equal(rh, r0)
    eng = mgn_amd.Engine(12, 7, 3, 128, 2, 3, Fe2=3)
    eng.set_graph(ms, mr, N)
    assert renumbered(eng)
    assert eng.world_edges_dev(1, pos, rad) == s0.size
    _assert_world_edges(eng, s0, r0, "scattered grid")
    assert not np.array_equal(eng.edge_set_export(1)[0], s0)                              # (and that is another order than the host search's)
    eng.close()


# ---- static inputs ---------------------------------------------------------------------------------------------------------------------
def _model(c):
    cfg = cfg_dict(Fn=2 + c["depth"], Fe=c["dim"] + 1, mps=2)
    return cfg, make_params(cfg)


def _norm_objects(c):
    return (orc.NormMeanStd(np.array([1.0, 0.9]), np.array([0.31, 0.27])), orc.NormMinMax(0.0, 1.0),
            orc.NormMeanStd(c["ef"].mean(0), c["ef"].std(0)), orc.NormMeanStd(np.array([0.01, -0.02]), np.array([0.5, 0.4])))


def _engine(c, dtype, **kw):
    cfg, ps = _model(c)
    n_norm, t_norm, e_norm, o_norm = _norm_objects(c)
    (ns, nsh), (ts, tsh), (es, esh) = n_norm.affine(2), t_norm.affine(c["depth"]), e_norm.affine(c["dim"] + 1)
    eng = engine_for(cfg, dtype=dtype, **kw)
    eng.set_params(ps)
    eng.set_graph(c["s"], c["r"], c["N"], **({"mesh_pos": c["pos"]} if kw else {}))
    eng.set_norms(node=(np.concatenate([ns, ts]), np.concatenate([nsh, tsh])), edge=(es, esh), out=(o_norm.std, o_norm.mean))
    return eng


def _rhs(c, dtype, route, want_renumbered=None):
    """mgn_ode_step on static inputs built by the device kernels ("mesh") or handed over as the oracle's arrays rounded to float32 ("host")"""
    eng = _engine(c, dtype)
    if want_renumbered is not None:
        assert renumbered(eng) == want_renumbered
    if route == "mesh":
        eng.set_static_mesh(c["node_type"], c["type_min"], c["type_max"], c["pos"], c["val_mask"])
    else:
        eng.set_static(c["onehot"].astype(np.float32), c["ef"].astype(np.float32), c["val_mask"])
    out = eng.ode_step(c["x"])
    assert np.array_equal(eng.ode_step(c["x"]), out)
    eng.close()
    assert np.isfinite(out).all() and np.abs(out).max() > 0
    return out


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", list(gc.STATIC_CASES))
def test_set_static_mesh_bit_equals_set_static(name, dtype):
    """Both routes feed identical values to identical kernels (see the module docstring).  The case with types outside [type_min,
    type_max] pins today's behaviour: such a node's one-hot row is all zeros."""
    c = gc.static_case(name)
    assert np.array_equal(_rhs(c, dtype, "mesh"), _rhs(c, dtype, "host"))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", list(gc.STATIC_CASES))
def test_set_static_mesh_on_scattered_labels(name, dtype):
    """the `l2g` branch of k_one_hot and k_edge_features (a renumbered handle reads node types and positions through own_gid): bit-equal
    to mgn_set_static on the same handle, and the rows of the unscattered mesh, permuted -- up to the order of the sums, which the
    numbering changes (the bound of tests/test_gpu_renumber.py for the same comparison; bf16: of tests/test_gpu_graph_dev.py)"""
    c = gc.static_case(name)
    d, perm = gc.scattered(c)
    out = _rhs(d, dtype, "mesh", want_renumbered=True)
    assert np.array_equal(out, _rhs(d, dtype, "host", want_renumbered=True))
    plain = _rhs(c, dtype, "mesh")
    print(f"{name} {dtype}: scattered vs plain rel_max = {rel_max(out[perm], plain):.3e}")
    assert rel_max(out[perm], plain) <= (1e-5 if dtype == "f32" else 2e-2)


@pytest.mark.parametrize("name", list(gc.STATIC_CASES))
def test_set_static_mesh_meets_the_oracle_rhs(name):
    """fp32 against the float64 right-hand side on the float64 one-hot rows and features, at the bound of tests/test_gpu_graph_dev.py"""
    c = gc.static_case(name)
    cfg, ps = _model(c)
    ref = orc.ode_rhs(ps, cfg, c["x"], c["onehot"], c["ef"], c["s"], c["r"], *_norm_objects(c), c["val_mask"][:, None])
    out = _rhs(c, "f32", "mesh")
    print(f"{name}: rel_max to the oracle = {rel_max(out, ref):.3e}")
    assert rel_max(out, ref) <= 1e-5


def test_set_static_mesh_refusals_leave_the_handle_usable():
    c = gc.static_case("2-D, types 0..6")
    nt, pos, vm, x = c["node_type"], c["pos"], c["val_mask"], c["x"]
    eng = _engine(c, "f32")
    eng.set_static_mesh(nt, 0, 6, pos, vm)
    out = eng.ode_step(x)
    assert np.array_equal(out, _rhs(c, "f32", "host"))
    pos3 = np.concatenate([pos, pos[:, :1]], 1)
    for args in ((nt, 0, 7, pos, vm), (nt, 1, 6, pos, vm),           # Fn - O != depth
                 (nt, 0, 6, pos3, vm), (nt, 0, 6, pos[:, :1], vm),   # Fe != pos_dim + 1
                 (nt, 6, 0, pos, vm)):                               # type_max < type_min
        with pytest.raises(mgn_amd.MgnError) as ei:
            eng.set_static_mesh(*args)
        assert ei.value.code == -1
        assert np.array_equal(eng.ode_step(x), out)                  # the resident static inputs are still the ones of the last good call
    eng.set_static_mesh(nt, 0, 6, pos, vm)
    assert np.array_equal(eng.ode_step(x), out)
    eng.close()
    # a partitioned handle
    part = _engine(c, "f32", rank=0, nranks=2)
    own = part.owned_nodes()
    with pytest.raises(mgn_amd.MgnError) as ei:
        part.set_static_mesh(nt, 0, 6, pos, vm)
    assert ei.value.code == -3
    rng = np.random.default_rng(0)
    v0, e0 = rng.standard_normal((c["N"], 128)).astype(np.float32), rng.standard_normal((c["s"].size, 128)).astype(np.float32)
    part.latents_import(v0, e0)
    v1, _ = part.latents_export()
    assert 0 < own.size < c["N"] and np.array_equal(part.owned_nodes(), own) and np.array_equal(v1[own], v0[own])
    part.close()
    # a handle with two edge sets
    two = mgn_amd.Engine(9, 3, 2, 128, 2, 2, Fe2=3)
    two.set_params(orc.init_params(9, 3, 2, 128, 2, 2, 1234, 0.1, Fe2=3))
    two.set_graph(c["s"], c["r"], c["N"])
    with pytest.raises(mgn_amd.MgnError) as ei:
        two.set_static_mesh(nt, 0, 6, pos, vm)
    assert ei.value.code == -3
    s0, r0 = gc.dense_world_edges(pos, 0.11, c["s"], c["r"])
    assert two.world_edges_dev(1, pos, 0.11) == s0.size > 0
    sd, rd = two.edge_set_export(1)
    assert np.array_equal(sd, s0) and np.array_equal(rd, r0)
    two.close()


# ---- triangles -------------------------------------------------------------------------------------------------------------------------
def test_triangles_to_edges_dev_every_soup():
    eng = engine_for(cfg_dict(mps=1))
    for name, cells in gc.SOUPS.items():
        so, ro = orc.triangles_to_edges(cells)
        s, r = eng.triangles_to_edges_dev(cells)
        assert np.array_equal(s, so) and np.array_equal(r, ro), name
    # cells and outputs as device tensors
    cells = gc.SOUPS["C = 86"]
    so, ro = orc.triangles_to_edges(cells)
    cap = 6 * cells.shape[0]
    tc = torch.from_numpy(cells.copy()).cuda()
    ts, tr = torch.full((cap,), -7, dtype=torch.int32, device="cuda"), torch.full((cap,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    n = C.c_int64()
    assert eng.lib.mgn_triangles_to_edges_dev(eng.h, tc.data_ptr(), cells.shape[0], ts.data_ptr(), tr.data_ptr(), cap, C.byref(n)) == 0
    assert n.value == so.size
    assert np.array_equal(ts.cpu().numpy()[:so.size], so) and np.array_equal(tr.cpu().numpy()[:so.size], ro)
    assert (ts.cpu().numpy()[so.size:] == -7).all() and (tr.cpu().numpy()[so.size:] == -7).all()       # nothing written past the count
    eng.close()
