"""The case table of tests/graph_prologue_cases.py against the host C++ prologue (csrc/graph_prologue.cpp), where no GPU is needed: the
table is well posed and the host side a sound second witness of tests/test_gpu_graph_dev_edges.py."""
import numpy as np
import pytest

import graph_prologue_cases as gc
import mgn_amd
import mgn_oracle as orc
from mgn_amd import MGN_DEVICE_NONE, Engine
from util import renumbered


@pytest.mark.parametrize("name", list(gc.WORLD_CASES))
def test_world_edges_host_equals_dense_search(lib_built, name):
    pos, rad, ms, mr = gc.WORLD_CASES[name]
    s0, r0 = gc.world_reference(name)
    s1, r1 = mgn_amd.world_edges_native(pos, rad, ms, mr)
    assert np.array_equal(s1, s0) and np.array_equal(r1, r0)
    s2, r2 = mgn_amd.world_edges_native(pos, rad, ms + 1, mr + 1, index_base=1)
    assert np.array_equal(s2, s0 + 1) and np.array_equal(r2, r0 + 1)


def test_world_edge_cases_are_what_they_claim():
    """the table itself: the counts of the 3-D lattice as literals, exclusion at distances equal to the radius, the one-way mesh list"""
    n = lambda name: gc.world_reference(name)[0].size
    assert tuple(n(f"lattice 3-D r={rad:g}") for rad in gc.LATTICE_RADII) == gc.LATTICE3_COUNTS == (0, 1764, 4788, 6516, 117306, 0)
    assert tuple(n(f"lattice 1-D r={rad:g}") for rad in gc.LATTICE_RADII) == (0, 12, 12, 12, 42, 0)       # 0.5 = two steps: excluded
    assert tuple(n(f"lattice 2-D r={rad:g}") for rad in gc.LATTICE_RADII) == (0, 168, 312, 312, 49 * 48, 0)
    assert n("37 identical points") == 37 * 36 and n("N = 1") == 0 and n("N = 2 far apart") == 0 and n("N = 2 near") == 2
    assert n("collinear, negative x") == 2 * (256 + 255)                                                   # one and two steps away, not three
    assert n("large box, tiny radius") == 0 and n("offset 1e4") > 100 and n("blob and outlier") > 1000
    s, r = gc.world_reference("coincident r=0.05")
    pos = gc.WORLD_CASES["coincident r=0.05"][0]
    assert s.size >= 400 and (np.abs(pos[s] - pos[r]).max(1) == 0).sum() == 400                           # 20 points x 5 x 4 pairs at distance 0
    assert gc.world_reference("coincident r=5")[0].size == 100 * 99
    assert (gc.world_reference("blob and outlier")[1] != 200).all()                                       # the outlier has no neighbour
    # the mesh list: one-way, with duplicates and self loops; a pair it excludes as (s, r) still comes out as (r, s)
    pos, rad, ms, mr = gc.WORLD_CASES["mesh list: one-way, duplicates, self loops"]
    key = lambda a, b: a.astype(np.int64) * 1000 + b
    listed = key(ms, mr)
    assert (ms == mr).sum() == 10 and listed.size - np.unique(listed).size == 20
    pairs = ms != mr
    assert pairs.sum() > 100 and not np.isin(key(mr[pairs], ms[pairs]), listed).any()                     # no pair is listed both ways
    s, r = gc.world_reference("mesh list: one-way, duplicates, self loops")
    out = key(s, r)
    assert not np.isin(listed, out).any() and np.isin(key(mr[pairs], ms[pairs]), out).all()
    full = key(*gc.dense_world_edges(pos, rad, gc.NONE, gc.NONE))
    assert np.array_equal(np.sort(np.concatenate([out, np.unique(listed[pairs])])), np.sort(full))               # and nothing else is missing


@pytest.mark.parametrize("name", list(gc.SOUPS))
def test_triangles_to_edges_host_equals_oracle(lib_built, name):
    cells = gc.SOUPS[name]
    s, r = mgn_amd.triangles_to_edges_native(cells)
    so, ro = orc.triangles_to_edges(cells)
    assert so.size and np.array_equal(s, so) and np.array_equal(r, ro)


@pytest.mark.parametrize("name", list(gc.STATIC_CASES))
def test_edge_features_host_are_the_rounded_float64_features(lib_built, name):
    c = gc.static_case(name)
    ef = c["ef"].astype(np.float32)
    assert np.array_equal(ef[:, :-1].astype(np.float64), c["ef"][:, :-1])                   # the differences are exact in float32 ...
    n2 = (c["ef"][:, :-1] ** 2).sum(1)
    assert np.array_equal(n2.astype(np.float32).astype(np.float64), n2)                     # ... and so is the sum of their squares
    assert (ef[:, :-1] < 0).any() and (ef[:, -1] > 0).all() and not np.array_equal(ef[:, -1].astype(np.float64), c["ef"][:, -1])
    assert np.array_equal(mgn_amd.edge_features_native(c["pos"], c["s"], c["r"]), ef)
    assert np.array_equal(mgn_amd.edge_features_native(c["pos"], c["s"] + 1, c["r"] + 1, index_base=1), ef)
    if not len(gc.STATIC_CASES[name][6]):
        assert np.array_equal(c["onehot"], orc.one_hot(c["node_type"], c["depth"], -c["type_min"]))
    d, perm = gc.scattered(c)
    assert np.array_equal(mgn_amd.edge_features_native(d["pos"], d["s"], d["r"]), ef)       # the same rows under scattered labels


def test_scattered_cases_are_renumbered(lib_built):
    """what the GPU tests of the `l2g` branch rest on, on host-only handles: mgn_set_graph renumbers every scattered case"""
    cases = [gc.scattered(gc.static_case(name))[0] for name in gc.STATIC_CASES]
    pos, _, ms, mr = gc.renumbered_world_case()
    cases.append(dict(s=ms, r=mr, N=pos.shape[0]))
    for d in cases:
        e = Engine(9, 3, 2, device=MGN_DEVICE_NONE)
        e.set_graph(d["s"], d["r"], d["N"])
        assert renumbered(e) and not np.array_equal(e.owned_nodes(), np.arange(d["N"]))
        e.close()
