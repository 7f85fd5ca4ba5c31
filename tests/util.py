"""Shared helpers for the parity tests (test infrastructure; may import the oracle)."""
import numpy as np

import mgn_amd
from mgn_amd import synth
import mgn_oracle as orc

# Stated tolerances: fp32 engine vs float64 oracle, max|d| / max|ref|
TOL_STEP = 2e-5       # latents after one processor step
TOL_15 = 1e-4         # latents / output after 15 steps
TOL_ROLLOUT = 1e-3    # relative L2 after a 100-step Euler rollout


def rel_max(a, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(a, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-30))


def cfg_dict(Fn=9, Fe=3, O=2, L=128, mps=15):
    return dict(Fn=Fn, Fe=Fe, O=O, L=L, hidden_layers=2, mps=mps)


def make_params(cfg, seed=1234, jitter=0.1):
    return orc.init_params(cfg["Fn"], cfg["Fe"], cfg["O"], cfg["L"], cfg["hidden_layers"], cfg["mps"], seed, jitter)


def small_mesh(nx=8, ny=6, seed=3):
    pos, cells = synth.grid_mesh(nx, ny, seed)
    s, r = synth.cells_to_edges(cells)
    return pos, s, r


def random_inputs(N, E, cfg, seed=0):
    rng = np.random.default_rng(seed)
    nf = rng.standard_normal((N, cfg["Fn"])).astype(np.float32)
    ef = rng.standard_normal((E, cfg["Fe"])).astype(np.float32)
    return nf, ef


def engine_for(cfg, **kw):
    return mgn_amd.Engine(cfg["Fn"], cfg["Fe"], cfg["O"], cfg["L"], cfg["hidden_layers"], cfg["mps"], **kw)


def set_kernel_path(path):
    """Force a kernel family (tests only): 0 auto, 1 LDS-resident persistent, 2 all-streaming, 3 cooperative."""
    lib = mgn_amd.load()
    lib.mgn_debug_kernel_path.restype = __import__("ctypes").c_int
    lib.mgn_debug_kernel_path.argtypes = [__import__("ctypes").c_int]
    return lib.mgn_debug_kernel_path(path)


def set_c16_row_tiles(rt):
    """16-edge tiles per block of the small-graph edge kernel (tests only): 0 chosen by size, 1..3 pinned.  Returns the old value."""
    lib = mgn_amd.load()
    lib.mgn_debug_c16_row_tiles.restype = __import__("ctypes").c_int
    lib.mgn_debug_c16_row_tiles.argtypes = [__import__("ctypes").c_int]
    return lib.mgn_debug_c16_row_tiles(rt)


def set_fp32_split(on):
    """Large fp32 launches: 1 = the split path (16-bit matrix cores at fp32 accuracy: the default), 0 = the fp32-MFMA kernels (tests
    only; any other value counts as 1).  Returns the old value."""
    lib = mgn_amd.load()
    lib.mgn_debug_fp32_split.restype = __import__("ctypes").c_int
    lib.mgn_debug_fp32_split.argtypes = [__import__("ctypes").c_int]
    return lib.mgn_debug_fp32_split(on)


def set_c16_split(on):
    """16-row cooperative kernels (small meshes) on the split path, bit mask: 1 = the edge kernel at two or three row tiles per block,
    2 = the node kernel (default 3 = both), 4 = the edge kernel at one row tile too; 0 = fp32-MFMA arithmetic.  Returns the old value."""
    lib = mgn_amd.load()
    lib.mgn_debug_c16_split.restype = __import__("ctypes").c_int
    lib.mgn_debug_c16_split.argtypes = [__import__("ctypes").c_int]
    return lib.mgn_debug_c16_split(on)


def set_split_f16(on):
    """Split path: 1 (default) = two fp16 pieces per operand, three piece products (k_edge_ring_h), 0 = three bf16 pieces, six products
    (k_edge_ring).  Returns the old value."""
    lib = mgn_amd.load()
    lib.mgn_debug_split_f16.restype = __import__("ctypes").c_int
    lib.mgn_debug_split_f16.argtypes = [__import__("ctypes").c_int]
    return lib.mgn_debug_split_f16(on)


def set_ringh_stream(on):
    """Split path on two fp16 pieces, edge step: 1 (default) = k_edge_ring_hs (every weight piece streamed, family codes 16 / 17),
    0 = k_edge_ring_h (13 / 14).  Returns the old value."""
    lib = mgn_amd.load()
    lib.mgn_debug_ringh_stream.restype = __import__("ctypes").c_int
    lib.mgn_debug_ringh_stream.argtypes = [__import__("ctypes").c_int]
    return lib.mgn_debug_ringh_stream(on)


def set_node_ring_hs(on):
    """Split path on two fp16 pieces, node side: 1 (default) = node MLP + projection in one k_node_ring_hs launch (family code 11),
    0 = k_node_split_h (10) + k_project_split_h.  Returns the old value."""
    lib = mgn_amd.load()
    lib.mgn_debug_node_ring_hs.restype = __import__("ctypes").c_int
    lib.mgn_debug_node_ring_hs.argtypes = [__import__("ctypes").c_int]
    return lib.mgn_debug_node_ring_hs(on)


def set_num_cus(n):
    """The CU count every size decision of the inference launches reads, and the one that scales the size rules of the training step
    (cooperative up to 8 n tiles, eight-tile blocks above 8 n, at most 4 n weight-gradient blocks, second-stream gradient sets up to
    8 n tiles) (tests only): 0 = the device's own -- for training: the literals 256 CUs stand for -- else a multiple of 8 from 8 up to the
    device's count.  Set it before the engine is created.  Returns the old value (0: no override), -1 if n is refused."""
    lib = mgn_amd.load()
    lib.mgn_debug_num_cus.restype = __import__("ctypes").c_int
    lib.mgn_debug_num_cus.argtypes = [__import__("ctypes").c_int]
    return lib.mgn_debug_num_cus(n)


def set_train_f16(on):
    """Training kernels at L = 128: 1 (default) = two fp16 pieces per operand, 0 = the fp32-MFMA forms (tests only).  Returns the old value."""
    lib = mgn_amd.load()
    lib.mgn_debug_train_f16.restype = __import__("ctypes").c_int
    lib.mgn_debug_train_f16.argtypes = [__import__("ctypes").c_int]
    return lib.mgn_debug_train_f16(on)


def train_regime(eng=None, reset=False):
    """mgn_debug_train_regime: launches of launch_mlp_fwd / launch_mlp_bwd / launch_lin2 since the last reset as
    (cooperative, four-tile streaming, eight-tile streaming, of these on fp16 pieces) under "fwd" / "bwd" / "lin2", and -- with an engine
    that has run a training step -- the plan of its training state: factored0 / factored1, gsets, need_gt, keep_steps, rows per block of
    the weight-gradient launches of the processor's node MLP (rpb_node) and edge MLPs (rpb_edge0 / rpb_edge1); -1 without one."""
    C = __import__("ctypes")
    lib = mgn_amd.load()
    lib.mgn_debug_train_regime.restype = C.c_int
    lib.mgn_debug_train_regime.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int32)]
    out = (C.c_int32 * 20)()
    assert lib.mgn_debug_train_regime(eng.h if eng is not None else None, int(reset), out) == 0
    v = list(out)
    d = {"fwd": tuple(v[0:4]), "bwd": tuple(v[4:8]), "lin2": tuple(v[8:12])}
    d.update(zip(("factored0", "factored1", "gsets", "need_gt", "keep_steps", "rpb_node", "rpb_edge0", "rpb_edge1"), v[12:20]))
    return d


def last_kernels():
    """(edge, node) family codes of the last launches (kernels.hip: launch_edge_step, launch_node_step; table in DESIGN.md)."""
    lib = mgn_amd.load()
    lib.mgn_debug_last_edge_kernel.restype = __import__("ctypes").c_int
    lib.mgn_debug_last_node_kernel.restype = __import__("ctypes").c_int
    return lib.mgn_debug_last_edge_kernel(), lib.mgn_debug_last_node_kernel()


def set_renumber(mode):
    """Node numbering policy of the next set_graph calls: 0 never, 1 auto (default), 2 always breadth-first (tests only)."""
    lib = mgn_amd.load()
    lib.mgn_debug_renumber.restype = __import__("ctypes").c_int
    lib.mgn_debug_renumber.argtypes = [__import__("ctypes").c_int]
    return lib.mgn_debug_renumber(mode)


def renumbered(eng):
    eng.lib.mgn_debug_renumbered.restype = __import__("ctypes").c_int
    eng.lib.mgn_debug_renumbered.argtypes = [__import__("ctypes").c_void_p]
    return bool(eng.lib.mgn_debug_renumbered(eng.h))


def scatter_labels(pos, s, r, seed=0):
    """The same mesh under arbitrary node labels (what DeepMind's trajectories carry; create_base_graph passes them through,
    reference src/graph.jl:30-36).  Returns (pos', s', r', perm) with perm[old] = new label; per-node arrays go x' = x[argsort(perm)]."""
    N = pos.shape[0]
    perm = np.random.default_rng(seed).permutation(N).astype(np.int32)
    return pos[np.argsort(perm)], perm[s], perm[r], perm
