"""The inputs and the plain references of tests/test_graph_prologue_host.py and tests/test_gpu_graph_dev_edges.py (host only: no torch, no
engine).  The graph prologue -- triangles to edges, one-hot node types, edge features, the world-edge search -- at the edges of its
input space: negative, coincident and collinear coordinates, distances equal to the radius, bounding boxes of zero extent, grids that
have to be coarsened, dim = 1, mesh-edge lists with duplicates, self loops and one-way entries, type ranges that do not start at 0.

Every world-edge case has N <= 350, so the dense float64 search is instant; every static mesh lies on a dyadic lattice (integers / 64),
so that every difference, square and sum of the edge features is exact in float32 and only the correctly rounded square root is left:
the float64 features rounded to float32 are then THE float32 features, bit for bit (a square root taken in 53 bits and rounded to 24
is the correctly rounded 24-bit one: 53 >= 2 * 24 + 2)."""
import numpy as np

import mgn_oracle as orc
from mgn_amd import synth
from util import scatter_labels

NONE = np.zeros(0, np.int32)


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---- world edges -----------------------------------------------------------------------------------------------------------------------
def dense_world_edges(pos, radius, ms, mr):
    """All ordered pairs (s, r), s != r, with |pos[s] - pos[r]|^2 < radius^2 that are not among the mesh edges (ms[i], mr[i]), 0-based;
    receiver-major with ascending senders.  Positions go to float64 from their float32 values, the radius from its float32 value; the
    squared distance is summed coordinate by coordinate, every product and every sum rounded once."""
    p = np.asarray(pos, np.float32).astype(np.float64)
    r2 = float(np.float32(radius)) ** 2
    d2 = np.zeros((p.shape[0], p.shape[0]))
    for d in range(p.shape[1]):
        dd = p[:, None, d] - p[None, :, d]
        d2 = d2 + dd * dd
    close = d2 < r2                                                   # [s][r]
    np.fill_diagonal(close, False)
    close[np.asarray(ms, np.int64), np.asarray(mr, np.int64)] = False
    r, s = np.nonzero(close.T)
    return s.astype(np.int32), r.astype(np.int32)


LATTICE_RADII = (0.25, 0.3, 0.375, 0.5, 10.0, 1e-3)
# {-3..3}^3 * 0.25, in steps: r = 0.25 reaches nothing (a distance of exactly one step is not < r); 0.3 the 2 * 3 * 6 * 49 axis neighbours;
# 0.375 the 2 * 6 * 36 * 7 face diagonals (sqrt 2 steps) too; 0.5 the 2 * 4 * 216 space diagonals (sqrt 3) too but not the pairs two steps
# apart (exactly 0.5); 10.0 all 343 * 342 pairs from ONE grid cell; 1e-3 nothing.
LATTICE3_COUNTS = (0, 1764, 4788, 6516, 117306, 0)


def _lattice(dim):
    ax = np.arange(-3, 4) * 0.25
    return np.stack(np.meshgrid(*([ax] * dim), indexing="ij"), -1).reshape(-1, dim).astype(np.float32)


def _mesh_list_case():
    """120 random 2-D points, the mesh-edge list drawn from the radius graph: about half of its pairs, ONE WAY only, 20 entries twice, 10 self
    loops.  A pair excluded as (s, r) and not listed as (r, s) must still come out as (r, s)."""
    rng = np.random.default_rng(120)
    pos = (rng.random((120, 2)) - 0.5).astype(np.float32)
    s, r = dense_world_edges(pos, 0.15, NONE, NONE)
    one_way = s < r
    pick = one_way & (rng.random(s.size) < 0.5)
    ms, mr = s[pick], r[pick]
    dup = rng.choice(ms.size, 20, replace=False)
    loops = rng.choice(120, 10, replace=False).astype(np.int32)
    ms, mr = np.concatenate([ms, ms[dup], loops]), np.concatenate([mr, mr[dup], loops])
    order = rng.permutation(ms.size)
    return pos, 0.15, ms[order].astype(np.int32), mr[order].astype(np.int32)


def _world_cases():
    c = {}
    for dim in (1, 2, 3):
        for rad in LATTICE_RADII:
            c[f"lattice {dim}-D r={rad:g}"] = (_lattice(dim), rad, NONE, NONE)
    c["1-D random, both signs"] = ((np.random.default_rng(1).random((300, 1)) * 3.0 - 2.0).astype(np.float32), 0.02, NONE, NONE)
    rng = np.random.default_rng(2005)
    coincident = np.repeat(rng.random((20, 3)), 5, axis=0)[rng.permutation(100)].astype(np.float32)
    c["coincident r=0.05"] = (coincident, 0.05, NONE, NONE)
    c["coincident r=5"] = (coincident, 5.0, NONE, NONE)
    c["37 identical points"] = (np.tile(np.array([[-0.3, 1.7]], np.float32), (37, 1)), 0.1, NONE, NONE)
    c["N = 1"] = (np.array([[0.5, -0.25, 2.0]], np.float32), 0.3, NONE, NONE)
    c["N = 2 far apart"] = (np.array([[-40.0, 3.0], [900.0, -7.0]], np.float32), 0.5, NONE, NONE)
    c["N = 2 near"] = (np.array([[-40.0, 3.0], [-40.25, 3.0]], np.float32), 0.5, NONE, NONE)
    line = np.zeros((257, 3), np.float32)
    line[:, 0] = -np.arange(257) / 64.0
    line[0, 0] = -0.0                                                # the origin's x is -0.0 ...
    line[100, 2] = -0.0                                              # ... and there is one -0.0 among the zeros of z (a zero-extent column)
    assert np.signbit(line[0, 0]) and np.signbit(line[100, 2]) and not np.signbit(line[1:, 1]).any()
    c["collinear, negative x"] = (line[np.random.default_rng(257).permutation(257)], 3.0 / 64.0, NONE, NONE)   # 3 steps away: excluded
    c["large box, tiny radius"] = ((np.random.default_rng(300).random((300, 3)) * 1000.0 - 500.0).astype(np.float32), 1e-3, NONE, NONE)
    blob = np.random.default_rng(200).normal(0.0, 0.01, (200, 2))
    c["blob and outlier"] = (np.concatenate([blob, [[50.0, 50.0]]], 0).astype(np.float32), 0.02, NONE, NONE)
    c["offset 1e4"] = ((np.random.default_rng(10000).random((300, 3)) + 1e4).astype(np.float32), 0.1, NONE, NONE)
    c["mesh list: one-way, duplicates, self loops"] = _mesh_list_case()
    for v in c.values():
        _ro(v[0], v[2], v[3])
        assert v[0].shape[0] <= 350
    return c


WORLD_CASES = _world_cases()
_dense = {}


def world_reference(name):
    """dense_world_edges of a case, computed once and shared (read-only)."""
    if name not in _dense:
        pos, rad, ms, mr = WORLD_CASES[name]
        _dense[name] = _ro(*dense_world_edges(pos, rad, ms, mr))
    return _dense[name]


def world_features(pos, s, r):
    """[pos[s] - pos[r] ; norm] in float64 from the float32 positions"""
    return orc.edge_features(np.asarray(pos, np.float32).astype(np.float64), s, r)


def renumbered_world_case():
    """A grid mesh under scattered node labels (mgn_set_graph renumbers it) whose world positions are the mesh positions: the radius
    reaches the second ring of neighbours, the mesh edges are excluded.  (pos, radius, ms, mr)"""
    pos, cells = synth.grid_mesh(17, 13, 5)
    s, r = synth.cells_to_edges(cells)
    pos, s, r, _ = scatter_labels(pos - np.float32(0.5), s, r, seed=3)
    pos, s, r = _ro(np.ascontiguousarray(pos, np.float32), s.astype(np.int32), r.astype(np.int32))
    return pos, 0.17, s, r


# ---- triangle soups --------------------------------------------------------------------------------------------------------------------
def _soups():
    rng = np.random.default_rng(86)
    t = np.array([3, 9, 4], np.int32)
    big = 2 ** 31 - 2
    c = {
        "degenerate triangles": np.array([[0, 1, 1], [2, 2, 3], [4, 5, 4], [6, 6, 6], [0, 1, 2], [1, 1, 0]], np.int32),
        "both orientations, repeated": np.stack([t, t[::-1], t, np.roll(t, 1), t[::-1], np.array([9, 4, 7], np.int32), t]),
        "C = 1": np.array([[7, 2, 5]], np.int32),
        "C = 85": rng.integers(0, 40, (85, 3)).astype(np.int32),          # 3 C = 255: one block of 256 threads, not full
        "C = 86": rng.integers(0, 40, (86, 3)).astype(np.int32),          # 3 C = 258: a second block of two threads
        "labels up to 2^31 - 2": np.array([[big, 0, big - 1], [big - 1, big, 5], [0, 5, big], [big, big - 1, 0]], np.int32),
        "one-based labels": (rng.integers(0, 30, (60, 3)) + 1).astype(np.int32),
    }
    _ro(*c.values())
    return c


SOUPS = _soups()


# ---- static meshes ---------------------------------------------------------------------------------------------------------------------
def one_hot_rows(node_type, type_min, type_max):
    """one_hot(node_type, depth = type_max - type_min + 1, offset = 1 - type_min) of the reference (src/graph.jl:26-27), 0-based: column
    type - type_min; a type outside [type_min, type_max] gives a row of zeros (the engine's behaviour; the reference would throw)."""
    t = np.asarray(node_type, np.int64)
    out = np.zeros((t.size, type_max - type_min + 1))
    ok = (t >= type_min) & (t <= type_max)
    out[np.nonzero(ok)[0], t[ok] - type_min] = 1.0
    return out


# name -> (nx, ny, dim, type_min, type_max, the types that occur, types outside the range to plant)
STATIC_CASES = {
    "2-D, types 0..6": (13, 11, 2, 0, 6, range(0, 7), ()),
    "3-D, types 1..7": (17, 13, 3, 1, 7, range(1, 8), ()),
    "2-D, types -2..4": (15, 5, 2, -2, 4, range(-2, 5), ()),
    "3-D, depth 1": (13, 7, 3, 5, 5, (5,), ()),
    "2-D, depth 7, first and last type only": (23, 13, 2, 0, 6, (0, 6), ()),
    "3-D, types -2..4, first and last only": (11, 5, 3, -2, 4, (-2, 4), ()),
    "2-D, types outside 0..6": (13, 11, 2, 0, 6, range(0, 7), (9, -1, 7)),
}
_static = {}


def static_case(name):
    """dict: pos [N][dim] on the lattice (integers / 64, negative ones too), cells, s, r, node_type, type_min, type_max, onehot [N][depth]
    float64, ef [E][dim + 1] float64 (both exactly representable in float32 up to the square root's rounding), val_mask, x [N][2]."""
    if name not in _static:
        nx, ny, dim, tmin, tmax, present, outside = STATIC_CASES[name]
        N = nx * ny
        assert 30 <= N <= 300 and N % 32
        _, cells = synth.grid_mesh(nx, ny, N)                          # the topology only
        s, r = synth.cells_to_edges(cells)
        rng = np.random.default_rng(7 * N + dim)
        iy, ix = np.divmod(np.arange(N), nx)
        cols = [4 * (ix - nx // 2) + rng.integers(-1, 2, N), 4 * (iy - ny // 2) + rng.integers(-1, 2, N)]   # whole lattice steps of jitter
        if dim == 3:
            cols.append(rng.integers(-6, 7, N))
        pos = (np.stack(cols, 1) / 64.0).astype(np.float32)
        assert np.array_equal(pos.astype(np.float64) * 64.0, np.stack(cols, 1)) and (pos < 0).any() and (pos > 0).any()
        present = np.array(list(present), np.int32)
        node_type = present[rng.integers(0, present.size, N)]
        node_type[rng.choice(N, present.size, replace=False)] = present           # every one of them occurs
        planted = rng.choice(N, len(outside), replace=False)
        node_type[planted] = outside
        onehot = one_hot_rows(node_type, tmin, tmax)
        assert (onehot.sum(1) == 0).sum() == len(outside)
        ef = orc.edge_features(pos.astype(np.float64), s, r)
        d = dict(pos=pos, cells=cells, s=s.astype(np.int32), r=r.astype(np.int32), N=N, dim=dim, node_type=node_type.astype(np.int32),
                 type_min=tmin, type_max=tmax, depth=tmax - tmin + 1, onehot=onehot, ef=ef, planted=planted,
                 val_mask=(rng.random(N) < 0.8).astype(np.float32), x=(rng.standard_normal((N, 2)) * 0.3 + 1.0).astype(np.float32))
        _ro(*(v for v in d.values() if isinstance(v, np.ndarray)))
        _static[name] = d
    return _static[name]


def scattered(case, seed=2):
    """The same mesh under arbitrary node labels: (dict with the keys of static_case, perm) with perm[old] = new label."""
    perm = np.random.default_rng(seed).permutation(case["N"]).astype(np.int32)
    inv = np.argsort(perm)
    d = dict(case)
    d.update(s=perm[case["s"]], r=perm[case["r"]])
    for k in ("pos", "node_type", "onehot", "val_mask", "x"):
        d[k] = case[k][inv]
    return d, perm
