"""The feature-width cases of tests/test_gpu_feature_widths.py and tests/test_feature_widths_host.py (test infrastructure; numpy and
the oracle only, no GPU).

The width rule (include/mgn_hip.h, mgn_config "Widths"): inference on ln_dims = MGN_LN_ROWS serves any Fn, Fe, Fe2, O >= 1; everything
that computes on the training kernels needs Fn, Fe, Fe2, O <= L.  IN_RANGE holds widths at the edges of that rule, WIDE the widths
above it (inference only: every training entry point refuses them).  Everything here is built once per case, shared and never written
to."""
import numpy as np

import mgn_oracle as orc
from mgn_amd import synth

F32 = np.float32
MPS = 2

# id: (Fn, Fe, O, L, hidden_layers)
IN_RANGE = {
    "min":      (1, 1, 1, 32, 2),          # one column everywhere; Fn == O: no one-hot, node_type_onehot = NULL
    "full32":   (32, 32, 4, 32, 2),        # inputs exactly L (in_rows = L); O = 4: the float4 path of k_save_error
    "out32":    (32, 31, 32, 32, 2),       # O = L = Fn (decoder out_cols = L, no one-hot); Fe = L - 1
    "cross64":  (33, 17, 5, 64, 2),        # across the 32-column tile, no multiples of 4; O = 5: two passes in k_save_error, scalar stores in k_datapoint_assemble
    "full64h3": (64, 64, 6, 64, 3),        # inputs = L on the general instantiations (two launch units)
    "edge128":  (127, 128, 7, 128, 2),     # L = 128 (fp16-piece training kernels by default); L - 1 and L
    "out128h1": (128, 128, 128, 128, 1),   # O = L = 128 at one hidden layer
}
# (Fn, Fe, O, L): a width above L, hidden_layers = 2
WIDE = [(33, 64, 33, 32), (65, 3, 2, 64), (64, 3, 2, 32)]


def wide_id(w):
    return "wide-Fn%d-Fe%d-O%d-L%d" % w


def cfg_of(case):
    """case: an id of IN_RANGE or a tuple of WIDE"""
    Fn, Fe, O, L, hl = IN_RANGE[case] if isinstance(case, str) else tuple(case) + (2,)
    return dict(Fn=Fn, Fe=Fe, O=O, L=L, hidden_layers=hl, mps=MPS)


def case_id(case):
    return case if isinstance(case, str) else wide_id(case)


ALL_FORWARD = list(IN_RANGE) + WIDE

_params = {}


def params(cfg):
    key = tuple(sorted(cfg.items()))
    if key not in _params:
        p = orc.init_params(cfg["Fn"], cfg["Fe"], cfg["O"], cfg["L"], cfg["hidden_layers"], cfg["mps"], seed=1234, ln_jitter=0.1,
                            Fe2=cfg.get("Fe2"))
        p.setflags(write=False)
        _params[key] = p
    return _params[key]


_meshes = {}


def mesh(kind="small"):
    """(senders, receivers, N): "small" = util.small_mesh(9, 7) (63 nodes, 316 edges); "resident8" = synth.random_graph(2083, 4137), above
    the cooperative range of the encoder / decoder launches at a test CU count of 8 (tests/test_gpu_encdec_stages.py)"""
    if kind not in _meshes:
        if kind == "small":
            pos, cells = synth.grid_mesh(9, 7, 3)
            s, r = synth.cells_to_edges(cells)
            N = pos.shape[0]
        else:
            N = 2083
            s, r = synth.random_graph(N, 4137, seed=N)
        for a in (s, r):
            a.setflags(write=False)
        _meshes[kind] = (s, r, int(N))
    return _meshes[kind]


class Problem:
    """Standard-normal inputs of a case on a mesh: nf, ef, target, mask, and for the right-hand side x, one-hot columns (random: any
    values serve), a 0/1 val_mask and non-trivial normalisers (scale in [0.5, 2], shift in [-1, 1] per feature)."""


_problems = {}


def problem(case, kind="small"):
    key = (case_id(case), kind)
    if key in _problems:
        return _problems[key]
    cfg = cfg_of(case)
    s, r, N = mesh(kind)
    E = s.size
    Fn, Fe, O = cfg["Fn"], cfg["Fe"], cfg["O"]
    rng = np.random.default_rng(sum(map(ord, key[0])) * 7919 + N)       # (a seed per case and mesh that no interpreter setting moves)
    P = Problem()
    P.cfg, P.s, P.r, P.N, P.E, P.ps = cfg, s, r, N, E, params(cfg)
    P.nf = rng.standard_normal((N, Fn)).astype(F32)
    P.ef = rng.standard_normal((E, Fe)).astype(F32)
    P.target = rng.standard_normal((N, O)).astype(F32)
    P.mask = np.sort(rng.choice(N, max(1, int(0.6 * N)), replace=False)).astype(np.int32)
    if Fn >= O:
        P.x = P.nf[:, :O].copy()
        P.onehot = P.nf[:, O:].copy() if Fn > O else None
        P.vm = (rng.random(N) < 0.7).astype(F32)
        P.lam = rng.standard_normal((N, O)).astype(F32)

        def affine(n):
            return rng.uniform(0.5, 2.0, n).astype(F32), rng.uniform(-1.0, 1.0, n).astype(F32)

        P.n_norm, P.e_norm, P.o_norm = affine(Fn), affine(Fe), affine(O)
    for a in vars(P).values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    _problems[key] = P
    return P


def rhs_inputs(P):
    """The float64 inputs of the model inside the right-hand side: [x ; one-hot] and ef through the normalisers' affine maps (the fp32
    scale and shift the engine holds, applied in float64)"""
    f64 = np.float64
    raw = P.x.astype(f64) if P.onehot is None else np.concatenate([P.x, P.onehot], 1).astype(f64)
    return raw * P.n_norm[0].astype(f64) + P.n_norm[1].astype(f64), P.ef.astype(f64) * P.e_norm[0].astype(f64) + P.e_norm[1].astype(f64)


def rhs_reference(P, nf64=None):
    """inverse(o_norm, orc.forward(normalised inputs)) * val_mask in float64"""
    nf, ef = rhs_inputs(P)
    out = orc.forward(P.ps, P.cfg, nf if nf64 is None else nf64, ef, P.s, P.r)
    return (out * P.o_norm[0].astype(np.float64) + P.o_norm[1].astype(np.float64)) * P.vm.astype(np.float64)[:, None]


class Affine:
    """An affine normaliser y = x * scale + shift as the oracle's ode_rhs / ode_vjp take one (NormMeanStd's interface): .std and .mean
    are those of its INVERSE when it is used as o_norm (out * std + mean)."""

    def __init__(self, scale, shift):
        self.scale, self.shift = np.asarray(scale, np.float64), np.asarray(shift, np.float64)
        self.std, self.mean = self.scale, self.shift

    def __call__(self, x):
        return x * self.scale + self.shift

    def inverse(self, y):
        return y * self.scale + self.shift

    def affine(self, dim):
        return self.scale[:dim], self.shift[:dim]


def oracle_norms(P):
    """(n_norm_fields, n_norm_type, e_norm, o_norm) of P for orc.ode_rhs / orc.ode_vjp"""
    O = P.cfg["O"]
    return (Affine(P.n_norm[0][:O], P.n_norm[1][:O]), Affine(P.n_norm[0][O:], P.n_norm[1][O:]), Affine(*P.e_norm), Affine(*P.o_norm))
