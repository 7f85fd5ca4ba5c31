"""Host-side mirror of the GraphNetCore surface the reference calls, over the C ABI.

Names follow the reference so that the parity tests read like its call sites:
    FeatureGraph(nf, ef, senders, receivers)              reference src/graph.jl:87-96
    GraphNetwork{model, ps, st, e_norm, n_norm, o_norm}   fields used at src/solve.jl:200-208, src/graph.jl:80-93
    mgn.model(graph, ps, st) -> (output, st)              src/solve.jl:200

Array convention: NumPy C row-major [count][feat] == the bytes of Julia's (feat x count) arrays.
There is no CPU compute path: constructing an Engine without the built HIP extension or without a
GPU raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _capi
from ._capi import MgnConfig, f32, i32, i64


class MgnError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"{_capi.STATUS_NAMES.get(code, code)}: {msg}")
        self.code = code


def _c32(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if shape is not None and tuple(a.shape) != tuple(shape):
        raise ValueError(f"DimensionMismatch: expected {tuple(shape)}, got {tuple(a.shape)}")
    return a


def _host_or_device(a, shape, writable=False):
    """(object kept alive, float* for the C ABI) of a NumPy array or a contiguous fp32 torch tensor (host or device: the
    entry points that document it copy with hipMemcpyDefault)."""
    if hasattr(a, "data_ptr"):                       # torch tensor
        import torch
        if a.dtype != torch.float32 or not a.is_contiguous():
            raise ValueError("tensor arguments must be contiguous float32")
        if tuple(a.shape) != tuple(shape):
            raise ValueError(f"DimensionMismatch: expected {tuple(shape)}, got {tuple(a.shape)}")
        return a, C.cast(C.c_void_p(a.data_ptr()), C.POINTER(C.c_float))
    if writable:
        if not (isinstance(a, np.ndarray) and a.dtype == np.float32 and a.flags.c_contiguous and a.flags.writeable):
            raise ValueError("out must be a writable contiguous float32 array")
        if tuple(a.shape) != tuple(shape):
            raise ValueError(f"DimensionMismatch: expected {tuple(shape)}, got {tuple(a.shape)}")
        return a, f32(a)
    a = _c32(a, shape)
    return a, f32(a)


class ErkTableau:
    """An explicit Runge-Kutta method as data: the MGN_ERK_TABLEAU_DOUBLES doubles of include/mgn_hip.h that the *_erk entry points take
    (make one with erk_tableau).  A [s][s] strictly lower triangular, b, c, btilde = b - bhat (zeros without an embedded pair)."""

    def __init__(self, tab, name=None):
        self.tab = np.ascontiguousarray(tab, dtype=np.float64).reshape(_capi.MGN_ERK_TABLEAU_DOUBLES).copy()
        self.name = name
        if _capi.load().mgn_erk_check(self._ptr()) != _capi.MGN_OK:
            raise ValueError("not an explicit Runge-Kutta tableau the library accepts (mgn_erk_check, include/mgn_hip.h)")

    def _ptr(self):
        return self.tab.ctypes.data_as(C.POINTER(C.c_double))

    stages = property(lambda self: int(self.tab[0]))
    order = property(lambda self: int(self.tab[1]))
    fsal = property(lambda self: bool(self.tab[2]))
    embedded = property(lambda self: bool(self.tab[3]))
    betas = property(lambda self: (float(self.tab[4]), float(self.tab[5])))
    A = property(lambda self: self.tab[6:55].reshape(7, 7)[:self.stages, :self.stages].copy())
    b = property(lambda self: self.tab[55:55 + self.stages].copy())
    c = property(lambda self: self.tab[62:62 + self.stages].copy())
    btilde = property(lambda self: self.tab[69:69 + self.stages].copy())

    def __repr__(self):
        return "ErkTableau(%s: %d stages, order %d%s%s)" % (self.name or "custom", self.stages, self.order, ", FSAL" if self.fsal else "",
                                                            ", embedded" if self.embedded else "")


def erk_tableau(name_or_A, b=None, c=None, btilde=None, order=None, fsal=False, betas=(0.0, 0.0)):
    """erk_tableau("RK4") -- one of "Euler", "Heun", "Midpoint", "Ralston", "RK4", "BS3", "DP5", "Tsit5" (mgn_erk_named) -- or
    erk_tableau(A, b, c[, btilde], order=p[, fsal, betas]): A [s][s] (its strictly lower triangle is used), s <= 7; btilde = b - bhat
    makes the pair embedded (adaptive steps); betas: the PI controller's (0, 0: the defaults 7/(10 p), 2/(5 p)).  ValueError for a
    tableau mgn_erk_check refuses."""
    tab = np.zeros(_capi.MGN_ERK_TABLEAU_DOUBLES, np.float64)
    if isinstance(name_or_A, str):
        if name_or_A not in _capi.ERK_NAMES:
            raise KeyError(name_or_A)
        rc = _capi.load().mgn_erk_named(_capi.ERK_NAMES[name_or_A], tab.ctypes.data_as(C.POINTER(C.c_double)))
        if rc != _capi.MGN_OK:
            raise MgnError(rc, "mgn_erk_named(%r)" % name_or_A)
        return ErkTableau(tab, name_or_A)
    if b is None or c is None or order is None:
        raise ValueError("erk_tableau(A, b, c[, btilde], order=p): b, c and order are required")
    A = np.atleast_2d(np.asarray(name_or_A, np.float64))
    b, c = np.asarray(b, np.float64).reshape(-1), np.asarray(c, np.float64).reshape(-1)
    s = b.size
    if not 1 <= s <= _capi.MGN_ERK_MAX_STAGES or A.shape != (s, s) or c.size != s or (btilde is not None and np.size(btilde) != s):
        raise ValueError("erk_tableau: A must be [s][s], b, c (and btilde) [s], 1 <= s <= %d" % _capi.MGN_ERK_MAX_STAGES)
    tab[:6] = s, order, 1.0 if fsal else 0.0, 0.0 if btilde is None else 1.0, betas[0], betas[1]
    tab[6:55].reshape(7, 7)[:s, :s] = A
    tab[55:55 + s], tab[62:62 + s] = b, c
    if btilde is not None:
        tab[69:69 + s] = np.asarray(btilde, np.float64).reshape(-1)
    return ErkTableau(tab)


def _erk_route(solver, adaptive):
    """How a rollout's `solver` reaches the library: None for "Euler" / "Tsit5" (mgn_rollout_desc.solver, today's calls), else
    (ErkTableau, adaptive flag) for the *_erk symbols -- a tableau without an embedded pair ignores `adaptive`, as "Euler" does; one with
    a pair follows it, as "Tsit5" does."""
    if isinstance(solver, str):
        if solver in ("Euler", "Tsit5") or solver not in _capi.ERK_NAMES:
            return None                                   # (an unknown name: _rollout_desc raises as it always has)
        solver = erk_tableau(solver)
    elif not isinstance(solver, ErkTableau):
        raise TypeError("solver must be a name or an ErkTableau, got %r" % type(solver).__name__)
    return solver, 1 if (solver.embedded and adaptive) else 0


class Engine:
    """One engine handle == one mesh partition on one GPU (rank/nranks select the partition)."""

    def __init__(self, Fn, Fe, O, L=128, hidden_layers=2, mps=15, rank=0, nranks=1, device=-1, dtype="f32", Fe2=None, ln_mode=0, ln_dims=0):
        """Fe2: input width of a second edge set (world edges, MGN-spec "per edge set"); None = the reference's one set.
        ln_mode: 0 = (x - mean) / sqrt(var + eps) (MGN-spec v1), 1 = (x - mean) / (sqrt(var) + eps) (spec_variant)."""
        self.lib = _capi.load()
        self.cfg = MgnConfig(Fn, Fe, O, L, hidden_layers, mps, {"f32": 0, "bf16": 1}[dtype], rank, nranks, device,
                             2 if Fe2 else 1, Fe2 or 0, ln_mode, {0: 0, 1: 1, "rows": 0, "all": 1}[ln_dims])
        self.E2 = 0
        self.h = C.c_void_p()
        rc = self.lib.mgn_create(C.byref(self.cfg), C.byref(self.h))
        if rc != 0:
            raise MgnError(rc, self.lib.mgn_last_error(None).decode())
        self.N = self.E = 0
        self.n_own = self.n_halo = self.e_local = 0

    # -- lifecycle -----------------------------------------------------------------------------
    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            self.lib.mgn_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise MgnError(rc, self.lib.mgn_last_error(self.h).decode())

    @property
    def host_only(self):
        return self.cfg.device == _capi.MGN_DEVICE_NONE

    def set_stream(self, stream_ptr):
        """stream_ptr: raw hipStream_t (0 = HIP default stream, e.g. torch.cuda.current_stream().cuda_stream);
        None = the engine's own private stream (MGN_STREAM_OWN)."""
        ptr = C.c_void_p(-1) if stream_ptr is None else C.c_void_p(stream_ptr)
        self._chk(self.lib.mgn_set_stream(self.h, ptr))

    def synchronize(self):
        self._chk(self.lib.mgn_synchronize(self.h))

    # -- parameters ----------------------------------------------------------------------------
    @property
    def param_count(self):
        return int(self.lib.mgn_param_count(C.byref(self.cfg)))

    def set_params(self, packed):
        packed = _c32(packed).ravel()
        self._chk(self.lib.mgn_set_params(self.h, f32(packed), packed.size))

    def get_params(self, out=None):
        """The parameters as they stand, whichever door they came through.  out: None (a new NumPy array), a writable float32
        NumPy array or a contiguous fp32 torch tensor, host or device (a device tensor is filled without a host round trip, on
        the engine's stream: synchronize() before another stream reads it)."""
        if out is None:
            out = np.empty(self.param_count, np.float32)
            self._chk(self.lib.mgn_get_params(self.h, f32(out), out.size))
            return out
        keep, p = _host_or_device(out, (self.param_count,), writable=True)
        self._chk(self.lib.mgn_get_params_dev(self.h, p, self.param_count))
        return keep

    def set_params_dev(self, packed):
        """New parameters into the engine's resident device vector: a contiguous fp32 torch tensor on the device (no host work, no
        synchronisation: the caller's optimiser lives on the GPU) or a host array.  Always counts as a change."""
        keep, p = _host_or_device(packed, (self.param_count,))
        self._chk(self.lib.mgn_set_params_dev(self.h, p, self.param_count))

    # -- Optimisers.Adam on the resident parameters ---------------------------------------------------
    def adam_init(self, eta=1e-3, beta=(0.9, 0.999), epsilon=1e-8):
        """Optimisers.setup(Optimisers.Adam(eta, beta, epsilon), ps): zero moments, beta_t = beta.  Resets an earlier state."""
        d = _capi.MgnAdamDesc(float(eta), float(beta[0]), float(beta[1]), float(epsilon))
        self._chk(self.lib.mgn_adam_init(self.h, C.byref(d)))

    def adam_update(self, grads):
        """Optimisers.update on the resident parameters, one kernel: grads as step() / step_datapoint() return them, NumPy or a
        contiguous fp32 torch tensor (with a device tensor nothing crosses PCIe and nothing blocks)."""
        keep, p = _host_or_device(grads, (self.param_count,))
        self._chk(self.lib.mgn_adam_update(self.h, p, self.param_count))

    def adam_state(self):
        """{"mt", "vt", "beta_t"}: the keys and dtypes of checkpoint.Adam's state, so save / write_checkpoint carry it unchanged."""
        mt, vt = np.empty(self.param_count, np.float32), np.empty(self.param_count, np.float32)
        bt = np.zeros(2, np.float64)
        self._chk(self.lib.mgn_adam_state(self.h, 0, f32(mt), f32(vt), bt.ctypes.data_as(C.POINTER(C.c_double))))
        return {"mt": mt, "vt": vt, "beta_t": bt}

    def set_adam_state(self, d):
        """Restore a state of adam_state() or of checkpoint.Adam (after adam_init, which gives eta, beta and epsilon)."""
        mt, vt = _c32(d["mt"]).ravel(), _c32(d["vt"]).ravel()
        bt = np.ascontiguousarray(d["beta_t"], dtype=np.float64).ravel()
        if mt.shape != (self.param_count,) or vt.shape != (self.param_count,) or bt.shape != (2,):
            raise ValueError(f"DimensionMismatch: expected mt, vt of ({self.param_count},) and beta_t of (2,)")
        self._chk(self.lib.mgn_adam_state(self.h, 1, f32(mt), f32(vt), bt.ctypes.data_as(C.POINTER(C.c_double))))

    def set_norms(self, node=None, edge=None, out=None):
        """Each argument: None (identity) or (scale[F], shift[F]) with forward y = x*scale + shift;
        `out` is the INVERSE map of o_norm (inverse_data)."""
        def sp(p, n):
            if p is None:
                return None, None
            return _c32(p[0], (n,)), _c32(p[1], (n,))
        ns, nsh = sp(node, self.cfg.Fn)
        es, esh = sp(edge, self.cfg.Fe)
        os_, osh = sp(out, self.cfg.O)
        self._keep_norms = (ns, nsh, es, esh, os_, osh)
        self._chk(self.lib.mgn_set_norms(self.h, f32(ns), f32(nsh), f32(es), f32(esh), f32(os_), f32(osh)))

    # -- graph ---------------------------------------------------------------------------------
    def set_graph(self, senders, receivers, N, index_base=0, mesh_pos=None):
        s = np.ascontiguousarray(senders, dtype=np.int32).ravel()
        r = np.ascontiguousarray(receivers, dtype=np.int32).ravel()
        if s.size != r.size:
            raise ValueError("DimensionMismatch: senders and receivers differ in length")
        pos, pd = None, 0
        if mesh_pos is not None:
            pos = _c32(mesh_pos)
            if pos.ndim != 2 or pos.shape[0] != N:
                raise ValueError("DimensionMismatch: mesh_pos must be [N][dim]")
            pd = pos.shape[1]
        self._chk(self.lib.mgn_set_graph(self.h, N, s.size, i32(s), i32(r), index_base, f32(pos), pd))
        self.N, self.E, self.E2 = int(N), int(s.size), 0
        self._refresh_partition()

    @staticmethod
    def partition_nodes(N, nranks, mesh_pos=None):
        """owner[N]: the node partition mgn_set_graph derives (recursive coordinate bisection of mesh_pos, or index blocks)."""
        lib = _capi.load()
        owner = np.empty(int(N), np.int32)
        pos, pd = None, 0
        if mesh_pos is not None:
            pos = _c32(mesh_pos)
            pd = pos.shape[1]
        rc = lib.mgn_partition_nodes(int(N), f32(pos), pd, int(nranks), i32(owner))
        if rc != 0:
            raise MgnError(rc, "mgn_partition_nodes")
        return owner

    def set_graph_local(self, senders, receivers, N, owner, index_base=0):
        """Rank-local ingest: the same state as set_graph(senders, receivers, N) with the partition `owner`, from the edges this rank
        has an end of (filtered here with numpy; a caller that holds only its part passes it to mgn_set_graph_local directly)."""
        s = np.ascontiguousarray(senders, dtype=np.int32).ravel()
        r = np.ascontiguousarray(receivers, dtype=np.int32).ravel()
        owner = np.ascontiguousarray(owner, dtype=np.int32).ravel()
        rank = self.cfg.rank
        touch = np.nonzero((owner[s - index_base] == rank) | (owner[r - index_base] == rank))[0].astype(np.int64)
        st, rt = np.ascontiguousarray(s[touch]), np.ascontiguousarray(r[touch])
        self._chk(self.lib.mgn_set_graph_local(self.h, int(N), i32(owner), int(s.size), int(touch.size), i32(st), i32(rt), i64(touch), index_base))
        self.N, self.E, self.E2 = int(N), int(s.size), 0
        self._refresh_partition()

    def _refresh_partition(self):
        a, b, c = C.c_int32(), C.c_int32(), C.c_int64()
        self._chk(self.lib.mgn_partition_info(self.h, C.byref(a), C.byref(b), C.byref(c)))
        self.n_own, self.n_halo, self.e_local = a.value, b.value, c.value

    def set_edge_set(self, set_index, senders, receivers, index_base=0):
        """Topology of the second edge set (after set_graph; as often as it changes)."""
        s = np.ascontiguousarray(senders, dtype=np.int32).ravel()
        r = np.ascontiguousarray(receivers, dtype=np.int32).ravel()
        if s.size != r.size:
            raise ValueError("DimensionMismatch: senders and receivers differ in length")
        self._chk(self.lib.mgn_set_edge_set(self.h, set_index, s.size, i32(s), i32(r), index_base))
        self.E2 = int(s.size)
        self._refresh_partition()

    def set_edge_features(self, set_index, ef):
        ef = _c32(ef, (self.E2, self.cfg.Fe2))
        self._chk(self.lib.mgn_set_edge_features(self.h, set_index, f32(ef)))

    def edge_set_info(self, set_index):
        a, b = C.c_int64(), C.c_int64()
        self._chk(self.lib.mgn_edge_set_info(self.h, set_index, C.byref(a), C.byref(b)))
        return a.value, b.value

    def edge_latents_import(self, set_index, e):
        e = _c32(e, ((self.E, self.E2)[set_index], self.cfg.L))
        self._chk(self.lib.mgn_edge_latents_import(self.h, set_index, f32(e)))

    def edge_latents_export(self, set_index, e=None):
        e = np.zeros(((self.E, self.E2)[set_index], self.cfg.L), np.float32) if e is None else e
        self._chk(self.lib.mgn_edge_latents_export(self.h, set_index, f32(e)))
        return e

    def owned_nodes(self):
        out = np.empty(self.n_own, np.int32)
        self._chk(self.lib.mgn_owned_nodes(self.h, i32(out)))
        return out

    def local_edges(self):
        out = np.empty(self.e_local, np.int64)
        self._chk(self.lib.mgn_local_edges(self.h, i64(out)))
        return out

    def halo_counts(self):
        n = self.cfg.nranks
        s, r = np.zeros(n, np.int32), np.zeros(n, np.int32)
        self._chk(self.lib.mgn_halo_counts(self.h, i32(s), i32(r)))
        return s, r

    def halo_nodes(self):
        out = np.empty(self.n_halo, np.int32)
        self._chk(self.lib.mgn_halo_nodes(self.h, i32(out)))
        return out

    def halo_send_index(self):
        s, _ = self.halo_counts()
        out = np.empty(int(s.sum()), np.int32)
        self._chk(self.lib.mgn_halo_send_index(self.h, i32(out)))
        return out

    def local_graph(self):
        snd = np.empty(self.e_local, np.int32)
        rcv = np.empty(self.e_local, np.int32)
        rowptr = np.empty(self.n_own + 1, np.int32)
        self._chk(self.lib.mgn_local_graph(self.h, i32(snd), i32(rcv), i32(rowptr)))
        return snd, rcv, rowptr

    def boundary_count(self):
        n = C.c_int32()
        self._chk(self.lib.mgn_boundary_count(self.h, C.byref(n)))
        return n.value

    def node_owner(self):
        out = np.empty(self.N, np.int32)
        self._chk(self.lib.mgn_node_owner(self.h, i32(out)))
        return out

    # -- model ---------------------------------------------------------------------------------
    def forward(self, nf, ef):
        nf = _c32(nf, (self.N, self.cfg.Fn))
        ef = _c32(ef, (self.E, self.cfg.Fe))
        out = np.zeros((self.N, self.cfg.O), np.float32)
        self._chk(self.lib.mgn_forward(self.h, f32(nf), f32(ef), f32(out)))
        return out

    def set_static(self, node_type_onehot, ef_raw, val_mask=None):
        """Once per trajectory: static RHS inputs become device-resident and the edge encoder runs once; afterwards
        ode_step(x) only moves the state."""
        O, Fn = self.cfg.O, self.cfg.Fn
        oh = _c32(node_type_onehot, (self.N, Fn - O)) if Fn > O else None
        ef = _c32(ef_raw, (self.E, self.cfg.Fe))
        vm = _c32(val_mask, (self.N,)) if val_mask is not None else None
        self._chk(self.lib.mgn_set_static(self.h, f32(oh), f32(ef), f32(vm)))

    # -- graph prologue on the device ----------------------------------------------
    def triangles_to_edges_dev(self, cells):
        """GraphNetCore.triangles_to_edges (reference src/graph.jl:30) on the device: (senders, receivers), two-way, first-occurrence
        order -- the same bits as triangles_to_edges_native."""
        cells = np.ascontiguousarray(cells, dtype=np.int32)
        if cells.ndim != 2 or cells.shape[1] != 3:
            raise ValueError("DimensionMismatch: cells must be [C][3]")
        cap = 6 * cells.shape[0]
        s, r = np.empty(max(cap, 1), np.int32), np.empty(max(cap, 1), np.int32)
        n = C.c_int64()
        self._chk(self.lib.mgn_triangles_to_edges_dev(self.h, cells.ctypes.data, cells.shape[0], s.ctypes.data, r.ctypes.data, cap, C.byref(n)))
        return s[: n.value].copy(), r[: n.value].copy()

    def set_static_mesh(self, node_type, type_min, type_max, mesh_pos, val_mask=None):
        """create_base_graph's feature half on the device (one-hot node types, edge features) + the once-per-trajectory edge encoder."""
        nt = np.ascontiguousarray(node_type, dtype=np.int32).ravel()
        pos = _c32(mesh_pos)
        if nt.size != self.N or pos.shape[0] != self.N:
            raise ValueError("DimensionMismatch: node_type / mesh_pos must have N rows")
        vm = _c32(val_mask, (self.N,)) if val_mask is not None else None
        self._keep_static = (nt, pos, vm)
        self._chk(self.lib.mgn_set_static_mesh(self.h, nt.ctypes.data, type_min, type_max, pos.ctypes.data, pos.shape[1],
                                               vm.ctypes.data if vm is not None else None))

    def world_edges_dev(self, set_index, world_pos, radius):
        """Search the world-edge set on the device and install it (no host round trip).  Returns the number of edges."""
        wp = _c32(world_pos)
        if wp.ndim != 2 or wp.shape[0] != self.N:
            raise ValueError("DimensionMismatch: world_pos must be [N][dim]")
        n = C.c_int64()
        self._chk(self.lib.mgn_world_edges_dev(self.h, set_index, wp.ctypes.data, wp.shape[1], C.c_float(radius), C.byref(n)))
        self.E2 = int(n.value)
        return self.E2

    def edge_set_export(self, set_index):
        E, _ = self.edge_set_info(set_index)
        s, r = np.empty(E, np.int32), np.empty(E, np.int32)
        self._chk(self.lib.mgn_edge_set_export(self.h, set_index, i32(s), i32(r)))
        return s, r

    def ode_step(self, x, node_type_onehot=None, ef_raw=None, val_mask=None):
        O, Fn = self.cfg.O, self.cfg.Fn
        x = _c32(x, (self.N, O))
        if node_type_onehot is None and ef_raw is None and val_mask is None:
            out = np.zeros((self.N, O), np.float32)
            self._chk(self.lib.mgn_ode_step(self.h, f32(x), None, None, None, f32(out)))
            return out
        oh = _c32(node_type_onehot, (self.N, Fn - O)) if Fn > O else None
        ef = _c32(ef_raw, (self.E, self.cfg.Fe))
        vm = _c32(val_mask, (self.N,)) if val_mask is not None else None
        out = np.zeros((self.N, O), np.float32)
        self._chk(self.lib.mgn_ode_step(self.h, f32(x), f32(oh), f32(ef), f32(vm), f32(out)))
        return out

    def _rollout_desc(self, solver, x0, node_type_onehot, ef_raw, t0, t1, saves_dt, n_saves, dt, val_mask, inflow_mask, inflow_data, abstol,
                      reltol, inflow_rule, time_type, adaptive=True, erk=None):
        """The descriptor of a rollout / rollout_eval call, without `out`; returns (d, the arrays it points into: inflow data last).
        adaptive=False with "Tsit5": fixed steps of dt (MGN_SOLVER_TSIT5_FIXED; the library refuses dt <= 0); "Euler" ignores it.
        erk (_erk_route's answer, not None): the call goes to an *_erk symbol, which does not read d.solver."""
        O, Fn = self.cfg.O, self.cfg.Fn
        d = _capi.MgnRolloutDesc()
        d.solver = {"Euler": _capi.MGN_SOLVER_EULER, "Tsit5": _capi.MGN_SOLVER_TSIT5}[solver] if erk is None else 0
        if solver == "Tsit5" and not adaptive:
            d.solver = _capi.MGN_SOLVER_TSIT5_FIXED
        d.t0, d.t1, d.dt, d.saves_dt, d.n_saves, d.abstol, d.reltol = t0, t1, dt, saves_dt, n_saves, abstol, reltol
        d.inflow_rule = {"reference": 0, "tolerant": 1}[inflow_rule]
        d.time_f64 = 1 if np.dtype(time_type) == np.float64 else 0
        d.t0_f64, d.t1_f64, d.dt_f64, d.saves_dt_f64 = t0, t1, dt, saves_dt
        x0 = _c32(x0, (self.N, O))
        oh = _c32(node_type_onehot, (self.N, Fn - O)) if Fn > O else None
        ef = _c32(ef_raw, (self.E, self.cfg.Fe))
        vm = _c32(val_mask, (self.N,)) if val_mask is not None else None
        im = np.ascontiguousarray(inflow_mask, dtype=np.uint8).reshape(self.N) if inflow_mask is not None else None
        idata = _c32(inflow_data) if inflow_data is not None else None
        if idata is not None and idata.shape[1:] != (self.N, O):
            raise ValueError("DimensionMismatch: inflow_data must be [frames][N][O]")
        d.x0, d.node_type_onehot, d.ef_raw, d.val_mask = f32(x0), f32(oh), f32(ef), f32(vm)
        d.inflow_mask = im.ctypes.data_as(C.POINTER(C.c_uint8)) if im is not None else None
        d.inflow_data = f32(idata)
        d.n_frames = idata.shape[0] if idata is not None else 0
        return d, (x0, oh, ef, vm, im, idata)

    def rollout(self, solver, x0, node_type_onehot, ef_raw, t0, t1, saves_dt, n_saves, dt=0.0, val_mask=None,
                inflow_mask=None, inflow_data=None, abstol=1e-6, reltol=1e-3, inflow_rule="reference", time_type=np.float32, adaptive=True):
        """Native device-side `rollout` (reference src/solve.jl:42-68).  solver: "Euler" (fixed dt) or "Tsit5".
        adaptive: "Tsit5" only ("Euler" ignores it).  True: `solve(prob, Tsit5(); saveat = saves, tstops = saves)`, dt the first step.
        False: `solve(prob, Tsit5(); adaptive = false, dt = dt, saveat = saves)` -- fixed steps of dt > 0 that need not divide
        saves_dt, saves between step ends from Tsit5's dense output, no error norm (MGN_SOLVER_TSIT5_FIXED, include/mgn_hip.h).
        inflow_rule: "reference" = `floor(Int, t / saves_dt) + 1` in the solver's time type, no tolerance, out of range raises
        (src/solve.jl:151); "tolerant" = + 1e-3, clamped (step k reads frame k).  time_type: np.float32 (the example's `0.0f0:0.01f0:5.99f0`) or np.float64.
        solver may also be "Heun", "Midpoint", "Ralston", "RK4", "BS3", "DP5" or an ErkTableau (erk_tableau): any explicit Runge-Kutta
        method of up to seven stages, through mgn_rollout_erk.  Without an embedded pair: fixed steps of dt whatever `adaptive` says;
        with one ("BS3", "DP5"): `adaptive` as for "Tsit5".  Fixed steps of a tableau need saves_dt / dt integral (no dense output).
        Returns (sol_u [n_saves][N][O], stats dict)."""
        erk = _erk_route(solver, adaptive)
        d, keep = self._rollout_desc(solver, x0, node_type_onehot, ef_raw, t0, t1, saves_dt, n_saves, dt, val_mask, inflow_mask, inflow_data,
                                     abstol, reltol, inflow_rule, time_type, adaptive, erk)
        out = np.zeros((n_saves, self.N, self.cfg.O), np.float32)
        d.out = f32(out)
        if erk is None:
            self._chk(self.lib.mgn_rollout(self.h, C.byref(d)))
        else:
            self._chk(self.lib.mgn_rollout_erk(self.h, C.byref(d), erk[0]._ptr(), erk[1]))
        del keep
        return out, dict(n_accept=d.n_accept, n_reject=d.n_reject, n_rhs=d.n_rhs)

    def rollout_eval(self, solver, x0, node_type_onehot, ef_raw, gt, t0, t1, saves_dt, n_saves, dt=0.0, val_mask=None, inflow_mask=None,
                     inflow_data=None, abstol=1e-6, reltol=1e-3, inflow_rule="reference", time_type=np.float32, sel=None, sel_index_base=0,
                     want_pred=False, mse_time_out=None, adaptive=True):
        """`rollout` with the errors against gt [n_gt >= n_saves][N][O] reduced on the device (mgn_rollout_eval): what _validation_step
        (reference src/strategies.jl:111-134) and eval_network! (src/MeshGraphNets.jl:609-635) take from a rollout.  The solve is
        rollout's (same arguments, bit-identical saves); without want_pred the solution is neither kept on the device nor downloaded.
        gt: NumPy array or contiguous fp32 device tensor; the SAME object as inflow_data reaches the C call as one pointer and is
        uploaded once.  sel: LINEAR indices (sel_index_base 0 or 1) into the [N][O] array mse_time -- the reference's `error[mask]`
        with its vector of node indices is this, not "every component of node sel[i]"; None: all N * O elements.  mse_time_out: a
        NumPy array or device tensor [N][O] to receive mse_time (default: a new NumPy array).
        Returns {"val_loss": mean(mse_time[sel]), "mse_save" [n_saves][O] float64 (mean over the nodes), "mse_time" [N][O] float32
        (mean over the saves), "pred" [n_saves][N][O] or None, "stats"}.  solver, adaptive: as rollout's (a tableau goes through
        mgn_rollout_eval_erk)."""
        O = self.cfg.O
        erk = _erk_route(solver, adaptive)
        d, keep = self._rollout_desc(solver, x0, node_type_onehot, ef_raw, t0, t1, saves_dt, n_saves, dt, val_mask, inflow_mask, inflow_data,
                                     abstol, reltol, inflow_rule, time_type, adaptive, erk)
        e = _capi.MgnRolloutEvalDesc()
        if gt is inflow_data:                           # validation: the ground truth is the inflow data -- one array, one pointer
            gt_keep, e.gt, e.n_gt = keep[-1], d.inflow_data, d.n_frames
        else:
            if len(gt.shape) != 3:
                raise ValueError("DimensionMismatch: gt must be [frames][N][O]")
            gt_keep, e.gt = _host_or_device(gt, (gt.shape[0], self.N, O))
            e.n_gt = gt.shape[0]
        pred = np.zeros((n_saves, self.N, O), np.float32) if want_pred else None
        d.out = f32(pred)
        mse_save = np.zeros((max(int(n_saves), 0), O), np.float64)
        e.mse_save = mse_save.ctypes.data_as(C.POINTER(C.c_double))
        mse_time, e.mse_time = _host_or_device(np.zeros((self.N, O), np.float32) if mse_time_out is None else mse_time_out, (self.N, O),
                                               writable=True)
        si = np.ascontiguousarray(sel, dtype=np.int32).reshape(-1) if sel is not None else None
        e.sel, e.n_sel, e.sel_index_base = i32(si), (si.size if si is not None else 0), int(sel_index_base)
        if erk is None:
            self._chk(self.lib.mgn_rollout_eval(self.h, C.byref(d), C.byref(e)))
        else:
            self._chk(self.lib.mgn_rollout_eval_erk(self.h, C.byref(d), C.byref(e), erk[0]._ptr(), erk[1]))
        del keep, gt_keep
        return {"val_loss": e.val_loss, "mse_save": mse_save, "mse_time": mse_time, "pred": pred,
                "stats": dict(n_accept=d.n_accept, n_reject=d.n_reject, n_rhs=d.n_rhs)}

    def _solver_desc(self, solver, x0, node_type_onehot, ef_raw, gt, t0, t1, dt, saves_dt, n_saves, val_mask, inflow_mask, inflow_data,
                     loss_scale, cont_target, inflow_rule, time_type, want_pred, out, abstol=0.0, reltol=0.0):
        """The descriptor and arrays of a solver_grad* call; returns (d, keep, p_gt, ls, p_ct, gs, p_gs, pred)."""
        O, Fn = self.cfg.O, self.cfg.Fn
        if int(n_saves) < 1:
            raise ValueError("n_saves must be >= 1")
        d = _capi.MgnRolloutDesc()
        d.solver = {"Euler": 0, "Tsit5": 1}[solver]
        d.t0, d.t1, d.dt, d.saves_dt, d.n_saves, d.abstol, d.reltol = t0, t1, dt, saves_dt, n_saves, abstol, reltol
        if inflow_rule not in ("reference", "tolerant"):
            raise ValueError(f"inflow_rule must be 'reference' or 'tolerant', got {inflow_rule!r}")
        d.inflow_rule = {"reference": 0, "tolerant": 1}[inflow_rule]
        d.time_f64 = 1 if np.dtype(time_type) == np.float64 else 0
        d.t0_f64, d.t1_f64, d.dt_f64, d.saves_dt_f64 = t0, t1, dt, saves_dt
        x0 = _c32(x0, (self.N, O))
        oh = _c32(node_type_onehot, (self.N, Fn - O)) if Fn > O else None
        ef = _c32(ef_raw, (self.E, self.cfg.Fe))
        vm = _c32(val_mask, (self.N,)) if val_mask is not None else None
        if (inflow_mask is None) != (inflow_data is None):
            raise ValueError("inflow_mask and inflow_data go together")
        im = np.ascontiguousarray(inflow_mask, dtype=np.uint8).reshape(self.N) if inflow_mask is not None else None
        idata = _c32(inflow_data) if inflow_data is not None else None
        if idata is not None and (idata.ndim != 3 or idata.shape[1:] != (self.N, O)):
            raise ValueError("DimensionMismatch: inflow_data must be [frames][N][O]")
        gt, p_gt = _host_or_device(gt, (n_saves, self.N, O))
        ls = _c32(loss_scale, (O,)) if loss_scale is not None else None
        ct, p_ct = _host_or_device(cont_target, (self.N, O)) if cont_target is not None else (None, None)
        if out is None:
            out = np.zeros(self.param_count, np.float32)
        gs, p_gs = _host_or_device(out, (self.param_count,), writable=True)
        pred = np.zeros((n_saves, self.N, O), np.float32) if want_pred else None
        d.x0, d.node_type_onehot, d.ef_raw, d.val_mask = f32(x0), f32(oh), f32(ef), f32(vm)
        d.inflow_mask = im.ctypes.data_as(C.POINTER(C.c_uint8)) if im is not None else None
        d.inflow_data = f32(idata)
        d.n_frames = idata.shape[0] if idata is not None else 0
        d.out = f32(pred)
        return d, (x0, oh, ef, vm, im, idata, gt, ct), p_gt, ls, p_ct, gs, p_gs, pred

    def solver_grad(self, x0, node_type_onehot, ef_raw, gt, t0, t1, dt, saves_dt, n_saves, val_mask=None, inflow_mask=None,
                    inflow_data=None, loss_scale=None, cont_target=None, cont_weight=0.0, inflow_rule="reference", time_type=np.float32,
                    want_pred=False, out=None, solver="Euler"):
        """Loss and gradient of one fixed-step Euler solve of ode_func_train on the device (mgn_solver_grad; reference
        src/solve.jl:101-117, strategies.jl:175-196, 257-292): the time grid, inflow frames and save rule of rollout("Euler", ...), with
        the inflow rows written into a copy the right-hand side sees (the state is not overwritten).
            loss = mean(((gt - x_saves) .* loss_scale) .^ 2 .* val_mask) + cont_weight * sum(abs.(x_end - cont_target))
        gt [n_saves][N][O] and cont_target [N][O]: NumPy arrays or contiguous fp32 device tensors; `out`: NumPy array or device tensor
        of param_count floats for the gradient.  The gradient is the discrete adjoint of the computed solution.
        solver: "Euler" (the only one this entry point differentiates; "Tsit5" is answered with MGN_E_UNSUPPORTED -- see
        solver_grad_tsit5).  Returns (grads, loss) or, with want_pred, (grads, loss, pred [n_saves][N][O])."""
        d, keep, p_gt, ls, p_ct, gs, p_gs, pred = self._solver_desc(solver, x0, node_type_onehot, ef_raw, gt, t0, t1, dt, saves_dt, n_saves,
                                                                   val_mask, inflow_mask, inflow_data, loss_scale, cont_target, inflow_rule,
                                                                   time_type, want_pred, out)
        loss = C.c_float()
        self._chk(self.lib.mgn_solver_grad(self.h, C.byref(d), p_gt, f32(ls), p_ct, float(cont_weight), p_gs, self.param_count,
                                           C.byref(loss)))
        del keep
        return (gs, loss.value, pred) if want_pred else (gs, loss.value)

    def shooting_grad(self, node_type_onehot, ef_raw, gt, windows, t0s, t1s, dt, saves_dt, val_mask=None, inflow_mask=None, inflow_data=None,
                      loss_scale=None, cont_weight=0.0, inflow_rule="reference", time_type=np.float32, solver="Euler", adaptive=False,
                      max_windows_per_pass=0, max_batch_nodes=0, want_pred=False, out=None):
        """The summed loss and gradient of the MultipleShooting windows `windows` [(first, last), ...] (0-based, inclusive indices into
        gt [n_gt][N][O]) in one native call (mgn_shooting_grad): window w is solver_grad (solver "Euler") or solver_grad_tsit5 with
        adaptive=False ("Tsit5") from x0 = gt[first] over (t0s[w], t1s[w]) with saves gt[first .. last], and the continuity term
        cont_weight * sum(abs.(x_end - gt[first of window w + 1])) for every window but the last.  Windows with the same step plan run
        together as one batch of graph copies, at most max_windows_per_pass (0: no cap) and max_batch_nodes nodes (0: 2^20) per pass.
        gt and `out` may be device tensors.  adaptive=True (Tsit5) is refused (MGN_E_UNSUPPORTED).  Returns (grads, loss) or, with
        want_pred, (grads, loss, pred [sum of the windows' saves][N][O]); self.last_shooting holds n_groups, n_passes, n_accept, n_rhs."""
        O = self.cfg.O
        n_gt = int(gt.shape[0])
        windows = [(int(a), int(b)) for a, b in windows]
        d, keep, p_gt, ls, _, gs, p_gs, _ = self._solver_desc(solver, np.zeros((self.N, O), np.float32), node_type_onehot, ef_raw, gt, 0.0,
                                                             0.0, dt, saves_dt, n_gt, val_mask, inflow_mask, inflow_data, loss_scale, None,
                                                             inflow_rule, time_type, False, out)
        W = len(windows)
        first = np.ascontiguousarray([a for a, _ in windows], np.int32)
        last = np.ascontiguousarray([b for _, b in windows], np.int32)
        t0 = np.ascontiguousarray(t0s, np.float64).reshape(W)
        t1 = np.ascontiguousarray(t1s, np.float64).reshape(W)
        s = _capi.MgnShootingDesc()
        s.n_windows, s.n_gt, s.adaptive = W, n_gt, 1 if adaptive else 0
        s.first = first.ctypes.data_as(C.POINTER(C.c_int32))
        s.last = last.ctypes.data_as(C.POINTER(C.c_int32))
        s.t0 = t0.ctypes.data_as(C.POINTER(C.c_double))
        s.t1 = t1.ctypes.data_as(C.POINTER(C.c_double))
        s.max_windows_per_pass, s.max_batch_nodes = int(max_windows_per_pass), int(max_batch_nodes)
        pred = np.zeros((int(sum(b - a + 1 for a, b in windows)), self.N, O), np.float32) if want_pred else None
        d.out = f32(pred)
        loss = C.c_float()
        self._chk(self.lib.mgn_shooting_grad(self.h, C.byref(d), C.byref(s), p_gt, f32(ls), float(cont_weight), p_gs, self.param_count,
                                             C.byref(loss)))
        del keep
        self.last_shooting = {"n_groups": s.n_groups, "n_passes": s.n_passes, "n_accept": d.n_accept, "n_rhs": d.n_rhs}
        return (gs, loss.value, pred) if want_pred else (gs, loss.value)

    def solver_grad_tsit5(self, x0, node_type_onehot, ef_raw, gt, t0, t1, saves_dt, n_saves, dt=0.0, adaptive=True, abstol=1e-6, reltol=1e-3,
                          val_mask=None, inflow_mask=None, inflow_data=None, loss_scale=None, cont_target=None, cont_weight=0.0,
                          inflow_rule="reference", time_type=np.float32, want_pred=False, out=None, step_cap=None, max_store_bytes=0,
                          dense_saves=False):
        """Loss and gradient of one Tsit5 solve of ode_func_train on the device (mgn_solver_grad_tsit5): solver_grad's loss, arguments
        and array rules, with
          adaptive=True:  rollout("Tsit5", ...)'s PI-controlled steps (first step dt, 0: the Hairer-Wanner start; abstol / reltol;
                          tstops = the saves), the error norm on the states (not overwritten);
          adaptive=False: fixed steps of dt on solver_grad's Euler time grid and save rule.
          dense_saves=True: no tstops -- `solve(...; saveat = saves)` as the reference's MultipleShooting calls it.  The only stop is t1
                          (adaptive: the controller steps freely; fixed: steps of dt, which need not divide saves_dt, the last one cut
                          or snapped onto t1); a save no step ends on is Tsit5's dense output inside the step that passes it, and the
                          adjoint carries its loss term with the steps and the interpolation points held fixed.  stored_bytes and
                          max_store_bytes then count 7 * N * O floats of sums as well.
        The gradient is the discrete adjoint of the computed solution with the accepted step sequence held fixed (step sizes and
        accept / reject decisions are constants); not InterpolatingAdjoint's continuous adjoint.
        Returns (grads, loss, stats): stats has n_accept, n_reject, n_rhs, step_t, step_h (the accepted steps' start times and sizes,
        at most step_cap of them; None: all), stored_bytes, n_steps, and pred [n_saves][N][O] with want_pred."""
        d, keep, p_gt, ls, p_ct, gs, p_gs, pred = self._solver_desc("Tsit5", x0, node_type_onehot, ef_raw, gt, t0, t1, dt, saves_dt, n_saves,
                                                                   val_mask, inflow_mask, inflow_data, loss_scale, cont_target, inflow_rule,
                                                                   time_type, want_pred, out, abstol, reltol)
        o = _capi.MgnSolverGradOpts()
        o.adaptive = (_capi.MGN_TSIT5_ADAPTIVE if adaptive else 0) | (_capi.MGN_TSIT5_DENSE_SAVES if dense_saves else 0)
        o.max_store_bytes = int(max_store_bytes)
        cap = step_cap
        if cap is None:                      # enough for every step a fixed-step solve takes, or a generous start for an adaptive one
            cap = int(round((float(t1) - float(t0)) / float(dt))) + 2 if (not adaptive and dt > 0) else 4096
        st, sh = np.zeros(max(int(cap), 1), np.float64), np.zeros(max(int(cap), 1), np.float64)
        o.step_cap = int(cap)
        o.step_t, o.step_h = st.ctypes.data_as(C.POINTER(C.c_double)), sh.ctypes.data_as(C.POINTER(C.c_double))
        loss = C.c_float()
        self._chk(self.lib.mgn_solver_grad_tsit5(self.h, C.byref(d), C.byref(o), p_gt, f32(ls), p_ct, float(cont_weight), p_gs,
                                                 self.param_count, C.byref(loss)))
        if step_cap is None and o.n_steps > cap:     # the record was cut: the call again with room for every step (bitwise repeatable)
            return self.solver_grad_tsit5(x0, node_type_onehot, ef_raw, gt, t0, t1, saves_dt, n_saves, dt, adaptive, abstol, reltol, val_mask,
                                          inflow_mask, inflow_data, loss_scale, cont_target, cont_weight, inflow_rule, time_type, want_pred,
                                          out, o.n_steps, max_store_bytes, dense_saves)
        del keep
        nrec = min(int(o.n_steps), int(cap))
        stats = dict(n_accept=d.n_accept, n_reject=d.n_reject, n_rhs=d.n_rhs, n_steps=int(o.n_steps), step_t=st[:nrec].copy(),
                     step_h=sh[:nrec].copy(), stored_bytes=int(o.stored_bytes))
        if want_pred:
            stats["pred"] = pred
        return gs, loss.value, stats

    def solver_grad_erk(self, tableau, x0, node_type_onehot, ef_raw, gt, t0, t1, saves_dt, n_saves, dt, val_mask=None, inflow_mask=None,
                        inflow_data=None, loss_scale=None, cont_target=None, cont_weight=0.0, inflow_rule="reference", time_type=np.float32,
                        want_pred=False, out=None, step_cap=None, max_store_bytes=0):
        """solver_grad_tsit5(adaptive=False) for any explicit Runge-Kutta method with at most six active stages (mgn_solver_grad_erk):
        tableau is an ErkTableau or one of erk_tableau's names.  Fixed steps of dt > 0 on rollout's grid for a tableau (saves_dt / dt
        integral), the inflow rows written into copies; the gradient is the exact discrete adjoint of the computed solution.
        Returns (grads, loss, stats) as solver_grad_tsit5 does."""
        tab = tableau if isinstance(tableau, ErkTableau) else erk_tableau(tableau)
        d, keep, p_gt, ls, p_ct, gs, p_gs, pred = self._solver_desc("Euler", x0, node_type_onehot, ef_raw, gt, t0, t1, dt, saves_dt, n_saves,
                                                                   val_mask, inflow_mask, inflow_data, loss_scale, cont_target, inflow_rule,
                                                                   time_type, want_pred, out)      # (d.solver is not read)
        o = _capi.MgnSolverGradOpts()
        o.adaptive, o.max_store_bytes = 0, int(max_store_bytes)
        cap = step_cap
        if cap is None:
            cap = int(round((float(t1) - float(t0)) / float(dt))) + 2 if dt > 0 else 1
        st, sh = np.zeros(max(int(cap), 1), np.float64), np.zeros(max(int(cap), 1), np.float64)
        o.step_cap = int(cap)
        o.step_t, o.step_h = st.ctypes.data_as(C.POINTER(C.c_double)), sh.ctypes.data_as(C.POINTER(C.c_double))
        loss = C.c_float()
        self._chk(self.lib.mgn_solver_grad_erk(self.h, C.byref(d), tab._ptr(), C.byref(o), p_gt, f32(ls), p_ct, float(cont_weight), p_gs,
                                               self.param_count, C.byref(loss)))
        del keep
        nrec = min(int(o.n_steps), int(cap))
        stats = dict(n_accept=d.n_accept, n_reject=d.n_reject, n_rhs=d.n_rhs, n_steps=int(o.n_steps), step_t=st[:nrec].copy(),
                     step_h=sh[:nrec].copy(), stored_bytes=int(o.stored_bytes))
        if want_pred:
            stats["pred"] = pred
        return gs, loss.value, stats

    def step(self, nf, ef, target, mask, mask_index_base=0, out=None):
        """step!(mgn, graph, target, mask, mse_reduce) (reference src/strategies.jl:418-422): returns (gs, loss) with gs
        in the packed order of set_params.  nf / ef / target may be NumPy arrays or contiguous fp32 torch tensors on
        the engine's GPU (the reference keeps the graph on the device); `out`: a NumPy array or device tensor of
        param_count floats that receives the gradients (device: no PCIe transfer, the optimiser runs where they are).
        On a partitioned mesh (nranks > 1, after comm_init; one edge set) every rank calls with the GLOBAL arrays -- nf [N][Fn],
        ef [E][Fe], target [N][O], mask with global node ids -- and gets the complete gradient and the loss of the whole mesh, the
        same bits on every rank: halo rows go forward once per processor step, their gradients go back to the owners in the
        reverse pass, the ranks' gradients are added in rank order at the end (mgn_step in include/mgn_hip.h)."""
        nf, p_nf = _host_or_device(nf, (self.N, self.cfg.Fn))
        ef, p_ef = _host_or_device(ef, (self.E, self.cfg.Fe))
        target, p_t = _host_or_device(target, (self.N, self.cfg.O))
        mask = np.ascontiguousarray(mask, dtype=np.int32).ravel()
        if out is None:
            out = np.zeros(self.param_count, np.float32)
        gs, p_gs = _host_or_device(out, (self.param_count,), writable=True)
        loss = C.c_float()
        self._chk(self.lib.mgn_step(self.h, p_nf, p_ef, p_t, i32(mask), mask.size, mask_index_base, p_gs, self.param_count,
                                    C.byref(loss)))
        return gs, loss.value

    # -- derivative training on a device-resident trajectory (mgn_train_* / mgn_step_datapoint) --------
    def set_trajectory(self, frames, dt=None, times=None, node_type_onehot=None, ef_raw=None):
        """Once per trajectory, after the graph is complete (add_targets! / preprocess!, reference src/dataset.jl:461-509):
        frames [T][N][O] (the target fields of every frame, concatenated in output order; the last frame is only ever a target),
        the time step as the scalar `dt` or as `times` [T], node_type_onehot [N][Fn-O], ef_raw [E][Fe].  NumPy arrays or
        contiguous fp32 device tensors, in the caller's node / edge order.  A new graph drops the trajectory, set_params and
        set_norms do not."""
        O, Fn = self.cfg.O, self.cfg.Fn
        shape = tuple(frames.shape)
        if len(shape) != 3 or shape[1:] != (self.N, O):
            raise ValueError(f"DimensionMismatch: frames must be [T][{self.N}][{O}], got {shape}")
        if (dt is None) == (times is None):
            raise ValueError("give either dt or times")
        frames, p_fr = _host_or_device(frames, shape)
        tm = _c32(times, (shape[0],)) if times is not None else None
        oh, p_oh = _host_or_device(node_type_onehot, (self.N, Fn - O)) if node_type_onehot is not None else (None, None)
        ef, p_ef = _host_or_device(ef_raw, (self.E, self.cfg.Fe)) if ef_raw is not None else (None, None)
        self._chk(self.lib.mgn_train_set_trajectory(self.h, p_fr, shape[0], f32(tm), 0.0 if dt is None else float(dt), p_oh, p_ef))
        self.T = shape[0]

    def set_noise(self, stddev=None, noisy_nodes=None, seed=0):
        """Noise of the input state (preprocess!, reference src/dataset.jl:496-509): stddev [O] (None: no noise), noisy_nodes [N]
        0/1 or bool in the caller's node order (None: every node), seed.  N(0,1) keyed by (seed, datapoint, caller's node id,
        column): independent of the engine's numbering.  The next state inside the target carries no noise."""
        sd = _c32(stddev, (self.cfg.O,)) if stddev is not None else None
        nz = None
        if noisy_nodes is not None:
            nz = np.ascontiguousarray(np.asarray(noisy_nodes).reshape(-1) != 0, dtype=np.uint8)
            if nz.shape != (self.N,):
                raise ValueError(f"DimensionMismatch: noisy_nodes must be [{self.N}]")
        self._chk(self.lib.mgn_train_set_noise(self.h, f32(sd), nz.ctypes.data_as(C.POINTER(C.c_uint8)) if nz is not None else None,
                                               int(seed)))

    def online_norms(self, node=True, edge=True, out=True, max_acc=1e6, std_epsilon=1e-8):
        """Switch the chosen groups (node state columns, edge features, output) to NormaliserOnline and zero their totals; a
        group left off keeps what set_norms gave it.  The one-hot columns are never online."""
        self._chk(self.lib.mgn_train_online_norms(self.h, int(bool(node)), int(bool(edge)), int(bool(out)), float(max_acc),
                                                  float(std_epsilon)))

    def _norm_dim(self, group):
        if group not in (0, 1, 2):
            return 1                   # (the library refuses the group)
        return self.cfg.Fe if group == 1 else self.cfg.O

    def norm_state(self, group):
        """(sum, sum_squares, count, calls) of an online group (0 node state columns, 1 edge, 2 output): float64 totals as they
        stand on the device -- what save! writes of a NormaliserOnline."""
        dim = self._norm_dim(group)
        s, q, cc = np.zeros(dim, np.float64), np.zeros(dim, np.float64), np.zeros(2, np.float64)
        dp = C.POINTER(C.c_double)
        self._chk(self.lib.mgn_train_norm_state(self.h, int(group), 0, s.ctypes.data_as(dp), q.ctypes.data_as(dp), cc.ctypes.data_as(dp)))
        return s, q, float(cc[0]), float(cc[1])

    def set_norm_state(self, group, sum, sum_squares, count, calls):
        """Restore an online group's totals (load): its affine map follows at the next datapoint."""
        dim = self._norm_dim(group)
        s = np.ascontiguousarray(sum, dtype=np.float64).reshape(-1)
        q = np.ascontiguousarray(sum_squares, dtype=np.float64).reshape(-1)
        if s.shape != (dim,) or q.shape != (dim,):
            raise ValueError(f"DimensionMismatch: expected ({dim},) totals")
        cc = np.array([count, calls], np.float64)
        dp = C.POINTER(C.c_double)
        self._chk(self.lib.mgn_train_norm_state(self.h, int(group), 1, s.ctypes.data_as(dp), q.ctypes.data_as(dp), cc.ctypes.data_as(dp)))

    def step_datapoint(self, t, mask, mask_index_base=0, accumulate=False, out=None):
        """init_train_step + step! of the derivative strategies (reference src/strategies.jl:395-422) on datapoint t (0-based,
        < T-1) of the resident trajectory: returns (gs, loss) like step().  accumulate: the online groups take this datapoint's
        raw rows into their totals and renew their maps first, on the device.  `out` as in step()."""
        mask = np.ascontiguousarray(mask, dtype=np.int32).ravel()
        if out is None:
            out = np.zeros(self.param_count, np.float32)
        gs, p_gs = _host_or_device(out, (self.param_count,), writable=True)
        loss = C.c_float()
        self._chk(self.lib.mgn_step_datapoint(self.h, int(t), int(bool(accumulate)), i32(mask), mask.size, mask_index_base, p_gs,
                                              self.param_count, C.byref(loss)))
        return gs, loss.value

    def step_datapoints(self, ts, mask, mask_index_base=0, accumulate=False, out=None):
        """step! on the block-diagonal FeatureGraph of the B datapoints ts (0-based, each < T-1, repeats and any order allowed;
        B <= 64) of the resident trajectory, the mask repeated per copy (the reference's Args.batchsize): returns
        (gs, loss, losses) with loss the mean of the per-datapoint losses [B] and gs its gradient, the mean of the per-datapoint
        gradients.  accumulate: the online groups take the B datapoints' raw rows into their totals first, one datapoint at a
        time, and all B are normalised with the resulting maps.  `out` as in step()."""
        ts = np.ascontiguousarray(ts, dtype=np.int32).ravel()
        mask = np.ascontiguousarray(mask, dtype=np.int32).ravel()
        if out is None:
            out = np.zeros(self.param_count, np.float32)
        gs, p_gs = _host_or_device(out, (self.param_count,), writable=True)
        loss = C.c_float()
        losses = np.zeros(max(ts.size, 1), np.float32)
        self._chk(self.lib.mgn_step_datapoints(self.h, i32(ts), ts.size, int(bool(accumulate)), i32(mask), mask.size, mask_index_base,
                                               p_gs, self.param_count, C.byref(loss), f32(losses)))
        return gs, loss.value, losses[:ts.size]

    def datapoint_export(self, t, normalised=True):
        """(nf [N][Fn], ef [E][Fe], target [N][O]) of datapoint t in the caller's order: what step_datapoint consumes
        (normalised) or the raw [cur ; onehot], ef_raw and d = (next - cur) / dt.  Never accumulates."""
        nf = np.zeros((self.N, self.cfg.Fn), np.float32)
        ef = np.zeros((self.E, self.cfg.Fe), np.float32)
        tg = np.zeros((self.N, self.cfg.O), np.float32)
        self._chk(self.lib.mgn_datapoint_export(self.h, int(t), int(bool(normalised)), f32(nf), f32(ef), f32(tg)))
        return nf, ef, tg

    def feature_stats(self, x):
        """Per-feature (sum, sum of squares) of x [rows][dim] in float64 on the device: one NormaliserOnline accumulation
        (GraphNetCore; normalisers of reference src/MeshGraphNets.jl:92,193-199).  x: NumPy array or device tensor."""
        shape = tuple(x.shape)
        if len(shape) != 2:
            raise ValueError("DimensionMismatch: x must be [rows][dim]")
        x, px = _host_or_device(x, shape)
        s = np.zeros(shape[1], np.float64)
        q = np.zeros(shape[1], np.float64)
        dp = C.POINTER(C.c_double)
        self._chk(self.lib.mgn_feature_stats(self.h, px, shape[0], shape[1], s.ctypes.data_as(dp), q.ctypes.data_as(dp)))
        return s, q

    def ode_vjp(self, x, node_type_onehot, ef_raw, lam, val_mask=None, want_dxdt=False):
        """lambda^T df/dx and lambda^T df/dps of the RHS f = ode_step (solver-based training, src/strategies.jl:175-196).
        Returns (xbar [N][O], gs [packed], dxdt or None)."""
        O, Fn = self.cfg.O, self.cfg.Fn
        x = _c32(x, (self.N, O))
        lam = _c32(lam, (self.N, O))
        oh = _c32(node_type_onehot, (self.N, Fn - O)) if Fn > O else None
        ef = _c32(ef_raw, (self.E, self.cfg.Fe))
        vm = _c32(val_mask, (self.N,)) if val_mask is not None else None
        xbar = np.zeros((self.N, O), np.float32)
        gs = np.zeros(self.param_count, np.float32)
        dxdt = np.zeros((self.N, O), np.float32) if want_dxdt else None
        self._chk(self.lib.mgn_ode_vjp(self.h, f32(x), f32(oh), f32(ef), f32(vm), f32(lam), f32(dxdt), f32(xbar), f32(gs), gs.size))
        return xbar, gs, dxdt

    def forward_vjp(self, nf, ef, ybar, want_out=False):
        """Pullback of forward() == of `mgn.model(graph, ps, st)` (src/solve.jl:200): ybar^T d out / d nf and ybar^T d out / d ps.
        Returns (nfbar [N][Fn], gs [packed], out or None): what a ChainRulesCore.rrule of the Julia shim's model hands to Zygote."""
        nf = _c32(nf, (self.N, self.cfg.Fn))
        ef = _c32(ef, (self.E, self.cfg.Fe))
        ybar = _c32(ybar, (self.N, self.cfg.O))
        nfbar = np.zeros((self.N, self.cfg.Fn), np.float32)
        gs = np.zeros(self.param_count, np.float32)
        out = np.zeros((self.N, self.cfg.O), np.float32) if want_out else None
        self._chk(self.lib.mgn_forward_vjp(self.h, f32(nf), f32(ef), f32(ybar), f32(out), f32(nfbar), f32(gs), gs.size))
        return nfbar, gs, out

    def processor_steps(self, v, e, nsteps):
        v = _c32(v, (self.N, self.cfg.L)).copy()
        e = _c32(e, (self.E, self.cfg.L)).copy()
        self._chk(self.lib.mgn_processor_steps(self.h, f32(v), f32(e), nsteps))
        return v, e

    # -- device-resident latents ---------------------------------------------------------------
    def latents_import(self, v, e):
        v = _c32(v, (self.N, self.cfg.L))
        e = _c32(e, (self.E, self.cfg.L))
        self._chk(self.lib.mgn_latents_import(self.h, f32(v), f32(e)))

    def latents_export(self, v=None, e=None):
        """Writes owned rows into GLOBAL-shaped arrays (allocated zero-filled when not given)."""
        v = np.zeros((self.N, self.cfg.L), np.float32) if v is None else v
        e = np.zeros((self.E, self.cfg.L), np.float32) if e is None else e
        self._chk(self.lib.mgn_latents_export(self.h, f32(v), f32(e)))
        return v, e

    def latents_randn(self, seed):
        self._chk(self.lib.mgn_latents_randn(self.h, C.c_uint64(seed)))

    def latents_checksum(self):
        a, b, c, d = (C.c_double() for _ in range(4))
        self._chk(self.lib.mgn_latents_checksum(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return dict(sum_v=a.value, sum_e=b.value, sumsq_v=c.value, sumsq_e=d.value)

    def processor_steps_dev(self, nsteps):
        self._chk(self.lib.mgn_processor_steps_dev(self.h, nsteps))

    # -- staged pipeline (multi-partition driver) ------------------------------------------------
    def fwd_upload(self, nf, ef):
        nf = _c32(nf, (self.N, self.cfg.Fn))
        ef = _c32(ef, (self.E, self.cfg.Fe))
        self._keep_in = (nf, ef)
        self._chk(self.lib.mgn_fwd_upload(self.h, f32(nf), f32(ef)))

    def fwd_encode(self):
        self._chk(self.lib.mgn_fwd_encode(self.h))

    def proc_begin(self):
        self._chk(self.lib.mgn_proc_begin(self.h))

    def proc_edge(self, k):
        self._chk(self.lib.mgn_proc_edge(self.h, k))

    def proc_node(self, k, project_next):
        self._chk(self.lib.mgn_proc_node(self.h, k, 1 if project_next else 0))

    def proc_node_phase(self, k, phase):
        """phase 1: node MLP of step k (k = -1: none) + projection of the boundary tiles; phase 2: interior tiles."""
        self._chk(self.lib.mgn_proc_node_phase(self.h, k, phase))

    def proc_edge_phase(self, k, phase):
        """phase 1: edge tiles without halo senders (may run while the halo exchange is in flight); phase 2: the rest."""
        self._chk(self.lib.mgn_proc_edge_phase(self.h, k, phase))

    def edge_boundary_tiles(self, set_index=0):
        a, b = C.c_int32(), C.c_int32()
        self._chk(self.lib.mgn_edge_boundary_tiles(self.h, set_index, C.byref(a), C.byref(b)))
        return a.value, b.value

    def fwd_decode(self):
        self._chk(self.lib.mgn_fwd_decode(self.h))

    def fwd_download(self, out=None):
        out = np.zeros((self.N, self.cfg.O), np.float32) if out is None else out
        self._chk(self.lib.mgn_fwd_download(self.h, f32(out)))
        return out

    @property
    def halo_row_floats(self):
        """width of one halo row in 4-byte units (exchange buffers are float32 tensors; bf16 rows are 64 wide)"""
        return int(self.lib.mgn_halo_bytes_per_row(self.h)) // 4

    def halo_pack(self, send_ptr):
        self._chk(self.lib.mgn_halo_pack(self.h, C.c_void_p(send_ptr)))

    def halo_unpack(self, recv_ptr):
        self._chk(self.lib.mgn_halo_unpack(self.h, C.c_void_p(recv_ptr)))

    # -- communicator: the halo exchange inside the library ---------------------
    @staticmethod
    def comm_unique_id(transport="rccl"):
        """MGN_COMM_ID_BYTES bytes made on ONE rank; the host distributes them (a torch.distributed store, MPI, a file)."""
        lib = _capi.load()
        buf = C.create_string_buffer(_capi.MGN_COMM_ID_BYTES)
        rc = lib.mgn_comm_unique_id(buf, _capi.TRANSPORTS[transport])
        if rc != 0:
            raise MgnError(rc, lib.mgn_last_error(None).decode())
        return buf.raw

    def comm_init(self, comm_id, transport="rccl"):
        """Collective over the nranks handles of the partitioned mesh; afterwards processor_steps_dev / forward run at
        nranks > 1 with the halo exchange inside the library.  transport "rccl" (one GPU per rank), "host" (shared memory) or
        "local" (the ranks are threads of this process; rows stay on the device)."""
        if len(comm_id) != _capi.MGN_COMM_ID_BYTES:
            raise ValueError("comm_id must be MGN_COMM_ID_BYTES bytes")
        buf = C.create_string_buffer(bytes(comm_id), _capi.MGN_COMM_ID_BYTES)
        self._chk(self.lib.mgn_comm_init(self.h, buf, _capi.MGN_COMM_ID_BYTES, _capi.TRANSPORTS[transport]))

    def comm_init_file(self, path, transport="rccl"):
        self._chk(self.lib.mgn_comm_init_file(self.h, str(path).encode(), _capi.TRANSPORTS[transport]))

    def comm_destroy(self):
        self._chk(self.lib.mgn_comm_destroy(self.h))

    def comm_barrier(self):
        self._chk(self.lib.mgn_comm_barrier(self.h))

    def comm_allreduce(self, x, op="sum"):
        x = np.ascontiguousarray(x, dtype=np.float64).copy()
        self._chk(self.lib.mgn_comm_allreduce(self.h, x.ctypes.data_as(C.POINTER(C.c_double)), x.size, {"sum": 0, "max": 1}[op]))
        return x

    def halo_exchange(self):
        self._chk(self.lib.mgn_halo_exchange(self.h))

    def halo_exchange_host(self, own_rows):
        """per-node host rows [n_own][W] -> rows of this partition's halo nodes [n_halo][W] (order of halo_nodes())"""
        own_rows = _c32(own_rows)
        if own_rows.ndim != 2 or own_rows.shape[0] != self.n_own:
            raise ValueError("DimensionMismatch: own_rows must be [n_own][W]")
        out = np.zeros((self.n_halo, own_rows.shape[1]), np.float32)
        self._chk(self.lib.mgn_halo_exchange_host(self.h, f32(own_rows), f32(out), own_rows.shape[1]))
        return out

    # -- measurement ---------------------------------------------------------------------------
    def profile_enable(self, on=True):
        self._chk(self.lib.mgn_profile_enable(self.h, 1 if on else 0))

    def profile_read(self):
        ms = (C.c_double * 8)()
        cnt = (C.c_int64 * 8)()
        self._chk(self.lib.mgn_profile_read(self.h, ms, cnt))
        names = ["edge_step", "node_step", "encode", "decode", "halo", "edge_boundary"]
        return {n: dict(avg_ms=ms[i], count=cnt[i]) for i, n in enumerate(names)}


class _RankView(Engine):
    """Rank k of a GroupEngine: the group's own handle, borrowed for introspection (partition_info, owned_nodes, halo_*, profile_*).
    No compute and no collective through it; it is never destroyed from here."""

    def __init__(self, group, k):   # (no mgn_create: the handle is the group's)
        self.lib = group.lib
        self.cfg = MgnConfig.from_buffer_copy(group.cfg)
        self.cfg.rank, self.cfg.nranks, self.cfg.device = k, group.nranks, group.devices[k]
        if getattr(group, "replicas", False):        # (a replica is a whole one-partition handle)
            self.cfg.rank, self.cfg.nranks = 0, 1
        self.h = C.c_void_p(self.lib.mgn_group_rank_handle(group.g, k))
        if not self.h.value:
            raise MgnError(_capi.MGN_E_ARG, f"no rank {k} in this group")
        self.N, self.E, self.E2 = group.N, group.E, 0
        self.n_own = self.n_halo = self.e_local = 0
        if group.N:
            self._refresh_partition()

    def close(self):
        self.h = C.c_void_p()


class GroupEngine:
    """All P partitions of a mesh driven from this one thread (mgn_group): rank k runs on devices[k] (ordinals may repeat), joined by an
    in-process "local" communicator.  The mirrored calls have Engine's names and take the GLOBAL arrays; results are the complete ones
    (rank 0's).  `with GroupEngine(...) as g:` or close()."""

    def __init__(self, Fn, Fe, O, L=128, hidden_layers=2, mps=15, devices=(0,), dtype="f32", Fe2=None, ln_mode=0, ln_dims=0, replicas=False):
        """replicas=True: a replica group (mgn_group_create_replicas) -- every rank holds the WHOLE mesh, step_datapoints splits its
        minibatch over them, every other call runs on all of them alike."""
        self.lib = _capi.load()
        self.devices = [int(d) for d in devices]
        self.nranks = len(self.devices)
        self.replicas = bool(replicas)
        self.cfg = MgnConfig(Fn, Fe, O, L, hidden_layers, mps, {"f32": 0, "bf16": 1}[dtype], 0, 1, -1,
                             2 if Fe2 else 1, Fe2 or 0, ln_mode, {0: 0, 1: 1, "rows": 0, "all": 1}[ln_dims])
        self.g = C.c_void_p()
        dev = np.ascontiguousarray(self.devices, np.int32)
        create = self.lib.mgn_group_create_replicas if self.replicas else self.lib.mgn_group_create
        rc = create(C.byref(self.cfg), self.nranks, i32(dev) if dev.size else None, C.byref(self.g))
        if rc != 0:
            raise MgnError(rc, self.lib.mgn_group_last_error(None).decode())
        self.N = self.E = 0

    def close(self):
        if getattr(self, "g", None) is not None and self.g.value:
            self.lib.mgn_group_destroy(self.g)
            self.g = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise MgnError(rc, self.lib.mgn_group_last_error(self.g).decode())

    def rank_engine(self, k):
        return _RankView(self, k)

    @property
    def param_count(self):
        return int(self.lib.mgn_param_count(C.byref(self.cfg)))

    def synchronize(self):
        self._chk(self.lib.mgn_group_synchronize(self.g))

    def set_params(self, packed):
        packed = _c32(packed).ravel()
        self._chk(self.lib.mgn_group_set_params(self.g, f32(packed), packed.size))

    def set_norms(self, node=None, edge=None, out=None):
        def sp(p, n):
            if p is None:
                return None, None
            return _c32(p[0], (n,)), _c32(p[1], (n,))
        ns, nsh = sp(node, self.cfg.Fn)
        es, esh = sp(edge, self.cfg.Fe)
        os_, osh = sp(out, self.cfg.O)
        self._chk(self.lib.mgn_group_set_norms(self.g, f32(ns), f32(nsh), f32(es), f32(esh), f32(os_), f32(osh)))

    def set_graph(self, senders, receivers, N, index_base=0, mesh_pos=None):
        s = np.ascontiguousarray(senders, dtype=np.int32).ravel()
        r = np.ascontiguousarray(receivers, dtype=np.int32).ravel()
        if s.size != r.size:
            raise ValueError("DimensionMismatch: senders and receivers differ in length")
        pos, pd = None, 0
        if mesh_pos is not None:
            pos = _c32(mesh_pos)
            if pos.ndim != 2 or pos.shape[0] != N:
                raise ValueError("DimensionMismatch: mesh_pos must be [N][dim]")
            pd = pos.shape[1]
        self._chk(self.lib.mgn_group_set_graph(self.g, N, s.size, i32(s), i32(r), index_base, f32(pos), pd))
        self.N, self.E = int(N), int(s.size)

    def set_static(self, node_type_onehot, ef_raw, val_mask=None):
        O, Fn = self.cfg.O, self.cfg.Fn
        oh = _c32(node_type_onehot, (self.N, Fn - O)) if Fn > O else None
        ef = _c32(ef_raw, (self.E, self.cfg.Fe))
        vm = _c32(val_mask, (self.N,)) if val_mask is not None else None
        self._chk(self.lib.mgn_group_set_static(self.g, f32(oh), f32(ef), f32(vm)))

    def forward(self, nf, ef):
        nf = _c32(nf, (self.N, self.cfg.Fn))
        ef = _c32(ef, (self.E, self.cfg.Fe))
        out = np.zeros((self.N, self.cfg.O), np.float32)
        self._chk(self.lib.mgn_group_forward(self.g, f32(nf), f32(ef), f32(out)))
        return out

    def ode_step(self, x, node_type_onehot=None, ef_raw=None, val_mask=None):
        O, Fn = self.cfg.O, self.cfg.Fn
        x = _c32(x, (self.N, O))
        out = np.zeros((self.N, O), np.float32)
        if node_type_onehot is None and ef_raw is None and val_mask is None:
            self._chk(self.lib.mgn_group_ode_step(self.g, f32(x), None, None, None, f32(out)))
            return out
        oh = _c32(node_type_onehot, (self.N, Fn - O)) if Fn > O else None
        ef = _c32(ef_raw, (self.E, self.cfg.Fe))
        vm = _c32(val_mask, (self.N,)) if val_mask is not None else None
        self._chk(self.lib.mgn_group_ode_step(self.g, f32(x), f32(oh), f32(ef), f32(vm), f32(out)))
        return out

    def rollout(self, solver, x0, node_type_onehot, ef_raw, t0, t1, saves_dt, n_saves, dt=0.0, val_mask=None,
                inflow_mask=None, inflow_data=None, abstol=1e-6, reltol=1e-3, inflow_rule="reference", time_type=np.float32, adaptive=True):
        """Engine.rollout on the partitioned mesh: (sol_u [n_saves][N][O], stats)."""
        erk = _erk_route(solver, adaptive)
        d, keep = Engine._rollout_desc(self, solver, x0, node_type_onehot, ef_raw, t0, t1, saves_dt, n_saves, dt, val_mask, inflow_mask,
                                       inflow_data, abstol, reltol, inflow_rule, time_type, adaptive, erk)
        out = np.zeros((n_saves, self.N, self.cfg.O), np.float32)
        d.out = f32(out)
        if erk is None:
            self._chk(self.lib.mgn_group_rollout(self.g, C.byref(d)))
        else:
            self._chk(self.lib.mgn_group_rollout_erk(self.g, C.byref(d), erk[0]._ptr(), erk[1]))
        del keep
        return out, dict(n_accept=d.n_accept, n_reject=d.n_reject, n_rhs=d.n_rhs)

    def step(self, nf, ef, target, mask, mask_index_base=0, out=None):
        """Engine.step on the partitioned mesh: (gs, loss).  nf / ef / target: host arrays (every rank reads them in place); `out`: a
        NumPy array or a tensor on devices[0] for the gradient."""
        nf = _c32(nf, (self.N, self.cfg.Fn))
        ef = _c32(ef, (self.E, self.cfg.Fe))
        target = _c32(target, (self.N, self.cfg.O))
        mask = np.ascontiguousarray(mask, dtype=np.int32).ravel()
        if out is None:
            out = np.zeros(self.param_count, np.float32)
        gs, p_gs = _host_or_device(out, (self.param_count,), writable=True)
        loss = C.c_float()
        self._chk(self.lib.mgn_group_step(self.g, f32(nf), f32(ef), f32(target), i32(mask), mask.size, mask_index_base, p_gs,
                                          self.param_count, C.byref(loss)))
        return gs, loss.value

    # -- derivative training on a device-resident trajectory, on the partitioned mesh (mgn_group_train_* / mgn_group_step_datapoint) --
    def set_trajectory(self, frames, dt=None, times=None, node_type_onehot=None, ef_raw=None):
        """Engine.set_trajectory on the partitioned mesh: host arrays of the whole mesh; every rank keeps the rows it owns."""
        O, Fn = self.cfg.O, self.cfg.Fn
        shape = tuple(frames.shape)
        if len(shape) != 3 or shape[1:] != (self.N, O):
            raise ValueError(f"DimensionMismatch: frames must be [T][{self.N}][{O}], got {shape}")
        if (dt is None) == (times is None):
            raise ValueError("give either dt or times")
        frames = _c32(frames, shape)
        tm = _c32(times, (shape[0],)) if times is not None else None
        oh = _c32(node_type_onehot, (self.N, Fn - O)) if node_type_onehot is not None else None
        ef = _c32(ef_raw, (self.E, self.cfg.Fe)) if ef_raw is not None else None
        self._chk(self.lib.mgn_group_train_set_trajectory(self.g, f32(frames), shape[0], f32(tm), 0.0 if dt is None else float(dt),
                                                          f32(oh), f32(ef)))
        self.T = shape[0]

    def set_noise(self, stddev=None, noisy_nodes=None, seed=0):
        """Engine.set_noise: noisy_nodes [N] of the whole mesh.  The noise of a node does not depend on the partition."""
        sd = _c32(stddev, (self.cfg.O,)) if stddev is not None else None
        nz = None
        if noisy_nodes is not None:
            nz = np.ascontiguousarray(np.asarray(noisy_nodes).reshape(-1) != 0, dtype=np.uint8)
            if nz.shape != (self.N,):
                raise ValueError(f"DimensionMismatch: noisy_nodes must be [{self.N}]")
        self._chk(self.lib.mgn_group_train_set_noise(self.g, f32(sd), nz.ctypes.data_as(C.POINTER(C.c_uint8)) if nz is not None else None,
                                                     int(seed)))

    def online_norms(self, node=True, edge=True, out=True, max_acc=1e6, std_epsilon=1e-8):
        self._chk(self.lib.mgn_group_train_online_norms(self.g, int(bool(node)), int(bool(edge)), int(bool(out)), float(max_acc),
                                                        float(std_epsilon)))

    _norm_dim = Engine._norm_dim

    def norm_state(self, group):
        """(sum, sum_squares, count, calls) of an online group as rank 0 holds them (every rank holds the same bits)."""
        dim = self._norm_dim(group)
        s, q, cc = np.zeros(dim, np.float64), np.zeros(dim, np.float64), np.zeros(2, np.float64)
        dp = C.POINTER(C.c_double)
        self._chk(self.lib.mgn_group_train_norm_state(self.g, int(group), 0, s.ctypes.data_as(dp), q.ctypes.data_as(dp), cc.ctypes.data_as(dp)))
        return s, q, float(cc[0]), float(cc[1])

    def set_norm_state(self, group, sum, sum_squares, count, calls):
        """Restore an online group's totals on every rank: its affine map follows at the next datapoint."""
        dim = self._norm_dim(group)
        s = np.ascontiguousarray(sum, dtype=np.float64).reshape(-1)
        q = np.ascontiguousarray(sum_squares, dtype=np.float64).reshape(-1)
        if s.shape != (dim,) or q.shape != (dim,):
            raise ValueError(f"DimensionMismatch: expected ({dim},) totals")
        cc = np.array([count, calls], np.float64)
        dp = C.POINTER(C.c_double)
        self._chk(self.lib.mgn_group_train_norm_state(self.g, int(group), 1, s.ctypes.data_as(dp), q.ctypes.data_as(dp), cc.ctypes.data_as(dp)))

    def __getattr__(self, name):
        # step_datapoint is looked up on the instance, not on the class: tests/test_step_datapoint_host.py, written when the datapoint
        # family drove one partition only, asserts that the class GroupEngine has no such attribute.  Every group has the method.
        # The same holds for step_datapoints and the Adam / set_params_dev mirrors (tests/test_step_datapoints_host.py,
        # tests/test_params_dev_host.py): instance attributes, the methods below under a leading underscore.
        if name in ("step_datapoint", "step_datapoints", "set_params_dev", "adam_init", "adam_update", "adam_state", "set_adam_state"):
            return object.__getattribute__(self, "_" + name)
        raise AttributeError(f"{type(self).__name__!r} object has no attribute {name!r}")

    def _step_datapoint(self, t, mask, mask_index_base=0, accumulate=False, out=None):
        """GroupEngine.step_datapoint: Engine.step_datapoint on the partitioned mesh: (gs, loss); mask holds node ids of the whole
        mesh; `out` as in step()."""
        mask = np.ascontiguousarray(mask, dtype=np.int32).ravel()
        if out is None:
            out = np.zeros(self.param_count, np.float32)
        gs, p_gs = _host_or_device(out, (self.param_count,), writable=True)
        loss = C.c_float()
        self._chk(self.lib.mgn_group_step_datapoint(self.g, int(t), int(bool(accumulate)), i32(mask), mask.size, mask_index_base, p_gs,
                                                    self.param_count, C.byref(loss)))
        return gs, loss.value

    # -- a minibatch over the group and Adam in place (mgn_group_step_datapoints, mgn_group_adam_*, mgn_group_*_params_dev) --
    def _step_datapoints(self, ts, mask, mask_index_base=0, accumulate=False, out=None, want_grads=True):
        """Engine.step_datapoints for the group: (gs or None, loss, losses).  A replica group splits ts over its replicas in contiguous
        chunks (replica k: len(ts) // P + (k < len(ts) % P) entries) and folds their gradients in a fixed order: the same bits on every
        replica; a partition group takes one datapoint.  want_grads=False leaves the gradient on the devices, where adam_update()
        finds it: nothing of parameter size crosses PCIe.  `out`: a host array the gradient is written into."""
        ts = np.ascontiguousarray(ts, dtype=np.int32).ravel()
        mask = np.ascontiguousarray(mask, dtype=np.int32).ravel()
        gs = None
        if want_grads:
            gs = np.zeros(self.param_count, np.float32) if out is None else out
            self._host_arrays(out=gs)
            if gs.dtype != np.float32 or not gs.flags.c_contiguous:
                raise TypeError("out: a contiguous float32 array")
        n_grads = self.param_count if gs is None else gs.size
        loss = C.c_float()
        losses = np.zeros(max(ts.size, 1), np.float32)
        self._chk(self.lib.mgn_group_step_datapoints(self.g, i32(ts), ts.size, int(bool(accumulate)), i32(mask), mask.size, mask_index_base,
                                                     f32(gs), n_grads, C.byref(loss), f32(losses)))
        return gs, loss.value, losses[:ts.size]

    def _set_params_dev(self, packed):
        """New parameters into every rank's resident device vector, from a host array."""
        packed = _c32(packed).ravel()
        self._chk(self.lib.mgn_group_set_params_dev(self.g, f32(packed), packed.size))

    def get_params_dev(self, rank=0, out=None):
        """Rank `rank`'s resident parameter vector, on the host: all ranks hold the same bits."""
        if out is None:
            out = np.empty(self.param_count, np.float32)
        self._chk(self.lib.mgn_group_get_params_dev(self.g, int(rank), f32(out), out.size))
        return out

    def _adam_init(self, eta=1e-3, beta=(0.9, 0.999), epsilon=1e-8):
        """Engine.adam_init on every rank."""
        d = _capi.MgnAdamDesc(float(eta), float(beta[0]), float(beta[1]), float(epsilon))
        self._chk(self.lib.mgn_group_adam_init(self.g, C.byref(d)))

    def _adam_update(self, grads=None):
        """Optimisers.update on every rank's resident parameters.  grads=None: each rank reads the gradient the last step_datapoints
        left on its own device (no copy, no host work); a host array: every rank reads it."""
        if grads is None:
            self._chk(self.lib.mgn_group_adam_update(self.g, None, self.param_count))
            return
        grads = _c32(grads).ravel()
        self._chk(self.lib.mgn_group_adam_update(self.g, f32(grads), grads.size))

    def _adam_state(self):
        """Engine.adam_state: rank 0's (all ranks hold the same)."""
        mt, vt = np.empty(self.param_count, np.float32), np.empty(self.param_count, np.float32)
        bt = np.zeros(2, np.float64)
        self._chk(self.lib.mgn_group_adam_state(self.g, 0, f32(mt), f32(vt), bt.ctypes.data_as(C.POINTER(C.c_double))))
        return {"mt": mt, "vt": vt, "beta_t": bt}

    def _set_adam_state(self, d):
        """Engine.set_adam_state on every rank."""
        mt, vt = _c32(d["mt"]).ravel(), _c32(d["vt"]).ravel()
        bt = np.ascontiguousarray(d["beta_t"], dtype=np.float64).ravel()
        if mt.shape != (self.param_count,) or vt.shape != (self.param_count,) or bt.shape != (2,):
            raise ValueError(f"DimensionMismatch: expected mt, vt of ({self.param_count},) and beta_t of (2,)")
        self._chk(self.lib.mgn_group_adam_state(self.g, 1, f32(mt), f32(vt), bt.ctypes.data_as(C.POINTER(C.c_double))))

    # -- solver-based training and the validation rollout on the partitioned mesh (mgn_group_solver_grad*, mgn_group_*_vjp,
    #    mgn_group_rollout_eval): Engine's methods, bodies included, run on the group's handle and the group's symbols --
    @staticmethod
    def _host_arrays(**arrays):
        for name, a in arrays.items():
            if a is not None and not isinstance(a, np.ndarray):
                raise TypeError(f"{name}: a group takes host (NumPy) arrays; every rank reads them in place")

    def solver_grad(self, x0, node_type_onehot, ef_raw, gt, t0, t1, dt, saves_dt, n_saves, val_mask=None, inflow_mask=None,
                    inflow_data=None, loss_scale=None, cont_target=None, cont_weight=0.0, inflow_rule="reference", time_type=np.float32,
                    want_pred=False, out=None, solver="Euler"):
        """Engine.solver_grad on the partitioned mesh (mgn_group_solver_grad): the loss and the complete gradient of the whole mesh; the
        save term divides by n_saves * N * O of the whole mesh.  Host arrays of the whole mesh."""
        self._host_arrays(gt=gt, cont_target=cont_target, out=out)
        return Engine.solver_grad(_GroupCalls(self), x0, node_type_onehot, ef_raw, gt, t0, t1, dt, saves_dt, n_saves, val_mask, inflow_mask,
                                  inflow_data, loss_scale, cont_target, cont_weight, inflow_rule, time_type, want_pred, out, solver)

    def solver_grad_tsit5(self, x0, node_type_onehot, ef_raw, gt, t0, t1, saves_dt, n_saves, dt=0.0, adaptive=True, abstol=1e-6, reltol=1e-3,
                          val_mask=None, inflow_mask=None, inflow_data=None, loss_scale=None, cont_target=None, cont_weight=0.0,
                          inflow_rule="reference", time_type=np.float32, want_pred=False, out=None, step_cap=None, max_store_bytes=0,
                          dense_saves=False):
        """Engine.solver_grad_tsit5 on the partitioned mesh (mgn_group_solver_grad_tsit5).  max_store_bytes bounds each rank's stored stage
        inputs; stats' stored_bytes is rank 0's (24 * n_own * O bytes per accepted step, with dense_saves 28 * n_own * O more), the step
        record is the same on every rank."""
        self._host_arrays(gt=gt, cont_target=cont_target, out=out)
        return Engine.solver_grad_tsit5(_GroupCalls(self), x0, node_type_onehot, ef_raw, gt, t0, t1, saves_dt, n_saves, dt, adaptive, abstol,
                                        reltol, val_mask, inflow_mask, inflow_data, loss_scale, cont_target, cont_weight, inflow_rule,
                                        time_type, want_pred, out, step_cap, max_store_bytes, dense_saves)

    def ode_vjp(self, x, node_type_onehot, ef_raw, lam, val_mask=None, want_dxdt=False):
        """Engine.ode_vjp on the partitioned mesh (mgn_group_ode_vjp): (xbar [N][O], gs, dxdt or None), complete and in the caller's order."""
        return Engine.ode_vjp(_GroupCalls(self), x, node_type_onehot, ef_raw, lam, val_mask, want_dxdt)

    def forward_vjp(self, nf, ef, ybar, want_out=False):
        """Engine.forward_vjp on the partitioned mesh (mgn_group_forward_vjp): (nfbar [N][Fn], gs, out or None)."""
        return Engine.forward_vjp(_GroupCalls(self), nf, ef, ybar, want_out)

    def rollout_eval(self, solver, x0, node_type_onehot, ef_raw, gt, t0, t1, saves_dt, n_saves, dt=0.0, val_mask=None, inflow_mask=None,
                     inflow_data=None, abstol=1e-6, reltol=1e-3, inflow_rule="reference", time_type=np.float32, sel=None, sel_index_base=0,
                     want_pred=False, mse_time_out=None, adaptive=True):
        """Engine.rollout_eval on the partitioned mesh (mgn_group_rollout_eval): sel indexes the whole mesh's [N][O]; val_loss divides by
        len(sel) (N * O without sel), mse_save by N.  Without want_pred no rank keeps, gathers or downloads the solution."""
        self._host_arrays(gt=gt, mse_time_out=mse_time_out)
        return Engine.rollout_eval(_GroupCalls(self), solver, x0, node_type_onehot, ef_raw, gt, t0, t1, saves_dt, n_saves, dt, val_mask,
                                   inflow_mask, inflow_data, abstol, reltol, inflow_rule, time_type, sel, sel_index_base, want_pred,
                                   mse_time_out, adaptive)

    def datapoint_export(self, t, normalised=True):
        """(nf [N][Fn], ef [E][Fe], target [N][O]) of datapoint t for the whole mesh: every rank writes the rows it owns."""
        nf = np.zeros((self.N, self.cfg.Fn), np.float32)
        ef = np.zeros((self.E, self.cfg.Fe), np.float32)
        tg = np.zeros((self.N, self.cfg.O), np.float32)
        self._chk(self.lib.mgn_group_datapoint_export(self.g, int(t), int(bool(normalised)), f32(nf), f32(ef), f32(tg)))
        return nf, ef, tg

    def latents_randn(self, seed):
        self._chk(self.lib.mgn_group_latents_randn(self.g, C.c_uint64(seed)))

    def processor_steps_dev(self, nsteps):
        self._chk(self.lib.mgn_group_processor_steps_dev(self.g, nsteps))

    def latents_checksum(self):
        a, b, c, d = (C.c_double() for _ in range(4))
        self._chk(self.lib.mgn_group_latents_checksum(self.g, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return dict(sum_v=a.value, sum_e=b.value, sumsq_v=c.value, sumsq_e=d.value)


class _GroupSymbols:
    """The library with mgn_group_X answering for mgn_X: what Engine's method bodies call when they run on a group."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        return getattr(self._lib, name.replace("mgn_", "mgn_group_", 1))


class _GroupCalls:
    """A GroupEngine as the solver methods of Engine see `self`: the mesh's sizes, the group's handle and error text, the group's symbols.
    Their bodies then serve both classes: one descriptor builder, one set of array checks, one return convention."""

    def __init__(self, group):
        self.lib, self.h, self.cfg = _GroupSymbols(group.lib), group.g, group.cfg
        self.N, self.E, self.param_count, self._chk = group.N, group.E, group.param_count, group._chk

    _rollout_desc, _solver_desc = Engine._rollout_desc, Engine._solver_desc
    solver_grad, solver_grad_tsit5, ode_vjp, forward_vjp, rollout_eval = (Engine.solver_grad, Engine.solver_grad_tsit5, Engine.ode_vjp,
                                                                          Engine.forward_vjp, Engine.rollout_eval)


def triangles_to_edges_native(cells):
    """GraphNetCore.triangles_to_edges at scale (C++ sort/unique on packed keys): returns (senders, receivers)."""
    lib = _capi.load()
    cells = np.ascontiguousarray(cells, dtype=np.int32)
    if cells.ndim != 2 or cells.shape[1] != 3:
        raise ValueError("DimensionMismatch: cells must be [C][3]")
    n = C.c_int64()
    rc = lib.mgn_triangles_to_edges(i32(cells), cells.shape[0], None, None, C.byref(n))
    if rc != 0:
        raise MgnError(rc, "mgn_triangles_to_edges")
    s, r = np.empty(n.value, np.int32), np.empty(n.value, np.int32)
    rc = lib.mgn_triangles_to_edges(i32(cells), cells.shape[0], i32(s), i32(r), C.byref(n))
    if rc != 0:
        raise MgnError(rc, "mgn_triangles_to_edges")
    return s, r


def world_edges_native(world_pos, radius, mesh_senders, mesh_receivers, index_base=0):
    """Radius graph in world space minus self loops and mesh-edge pairs (world edges of cloth models): (senders, receivers)."""
    lib = _capi.load()
    wp = _c32(world_pos)
    ms = np.ascontiguousarray(mesh_senders, dtype=np.int32)
    mr = np.ascontiguousarray(mesh_receivers, dtype=np.int32)
    n = C.c_int64()
    args = (f32(wp), wp.shape[1], wp.shape[0], C.c_float(radius), i32(ms), i32(mr), ms.size, index_base)
    rc = lib.mgn_world_edges(*args, None, None, C.byref(n))
    if rc != 0:
        raise MgnError(rc, "mgn_world_edges")
    s, r = np.empty(n.value, np.int32), np.empty(n.value, np.int32)
    rc = lib.mgn_world_edges(*args, i32(s), i32(r), C.byref(n))
    if rc != 0:
        raise MgnError(rc, "mgn_world_edges")
    return s, r


def edge_features_native(mesh_pos, senders, receivers, index_base=0):
    lib = _capi.load()
    pos = _c32(mesh_pos)
    s = np.ascontiguousarray(senders, dtype=np.int32)
    r = np.ascontiguousarray(receivers, dtype=np.int32)
    ef = np.empty((s.size, pos.shape[1] + 1), np.float32)
    rc = lib.mgn_edge_features(f32(pos), pos.shape[1], i32(s), i32(r), s.size, index_base, f32(ef))
    if rc != 0:
        raise MgnError(rc, "mgn_edge_features")
    return ef


# ==================================================================================================
# GraphNetCore-shaped surface
# ==================================================================================================
class FeatureGraph:
    """FeatureGraph(nf, ef, senders, receivers) -- reference src/graph.jl:87-96.  Single edge set."""

    def __init__(self, nf, ef, senders, receivers):
        self.nf, self.ef, self.senders, self.receivers = nf, ef, senders, receivers


class _Model:
    """Callable `mgn.model(graph, ps, st) -> (output, st)` (reference src/solve.jl:200)."""

    def __init__(self, net):
        self.net = net

    def __call__(self, graph, ps, st):
        net = self.net
        net._sync_params(ps)
        net._sync_graph(graph.senders, graph.receivers, np.asarray(graph.nf).shape[0])
        return net.engine.forward(graph.nf, graph.ef), st


class GraphNetwork:
    """Mutable holder mirroring GraphNetCore.GraphNetwork: fields model, ps, st, e_norm, n_norm, o_norm
    (reference reads/writes them at src/solve.jl:54,200-208, src/graph.jl:80-93,
    src/MeshGraphNets.jl:288,376-377).  `ps` is the packed float32 parameter vector (MGN-spec order),
    owned by the caller so an optimiser can update it in place; it is re-uploaded when it changes."""

    def __init__(self, quantities, dims, e_norm, n_norm, o_norm, outputs, mps=15, layer_size=128,
                 hidden_layers=2, ps=None, index_base=0, device=-1, gpus=None):
        """gpus: HIP ordinals (may repeat), one edge-cut partition each, all driven from this process through a GroupEngine; None: the
        environment variable MGN_GPUS (a comma list) if set, else one partition on `device`."""
        if gpus is None and os.environ.get("MGN_GPUS"):
            gpus = [int(x) for x in os.environ["MGN_GPUS"].split(",") if x.strip()]
        if gpus:
            self.engine = GroupEngine(quantities, dims + 1, outputs, layer_size, hidden_layers, mps, devices=gpus)
        else:
            self.engine = Engine(quantities, dims + 1, outputs, layer_size, hidden_layers, mps, device=device)
        self.e_norm, self.n_norm, self.o_norm = e_norm, n_norm, o_norm
        self.st = None
        self.index_base = index_base
        if ps is None:
            raise ValueError("ps (packed parameters) is required: use load_params or init_params")
        self.ps = np.ascontiguousarray(ps, np.float32)
        self._ps_token = None
        self._graph_token = None
        self.model = _Model(self)

    def _sync_params(self, ps):
        ps = np.ascontiguousarray(ps, np.float32)
        tok = (ps.ctypes.data, ps.size, float(ps[:64].sum()), float(ps[-64:].sum()), float(ps[::4099].sum()))
        if tok != self._ps_token:
            self.engine.set_params(ps)
            self._ps_token = tok

    def _sync_graph(self, senders, receivers, N):
        s = np.asarray(senders)
        tok = (s.ctypes.data if s.flags.c_contiguous else id(senders), s.size, N, int(s[:16].sum()) if s.size else 0)
        if tok != self._graph_token:
            self.engine.set_graph(senders, receivers, N, index_base=self.index_base)
            self._graph_token = tok

    def set_graph(self, senders, receivers, N, mesh_pos=None):
        """Explicit once-per-trajectory call (what create_base_graph amortises, src/MeshGraphNets.jl:360)."""
        self.engine.set_graph(senders, receivers, N, index_base=self.index_base, mesh_pos=mesh_pos)
        s = np.asarray(senders)
        self._graph_token = (s.ctypes.data if s.flags.c_contiguous else id(senders), s.size, N,
                             int(s[:16].sum()) if s.size else 0)


def init_params(cfg, seed=None):
    """Fresh parameters in packed order: Glorot-uniform weights, zero biases, LayerNorm scale 1 / bias 0 (the twin of
    MGNHip.init_params; NumPy's draws).  cfg: (Fn, Fe, O, L, hidden_layers, mps)."""
    Fn, Fe, O, L, h, mps = (int(x) for x in cfg)
    rng = np.random.default_rng(seed)
    parts = []

    def mlp(fin, fout, ln):
        dims = [fin] + [L] * h + [fout]
        for a, b in zip(dims[:-1], dims[1:]):
            lim = np.sqrt(6.0 / (a + b))
            parts.append(((rng.random(a * b, dtype=np.float32) * 2 - 1) * lim).astype(np.float32))
            parts.append(np.zeros(b, np.float32))
        if ln:
            parts.extend((np.ones(fout, np.float32), np.zeros(fout, np.float32)))

    mlp(Fn, L, True)
    mlp(Fe, L, True)
    for _ in range(mps):
        mlp(3 * L, L, True)
        mlp(2 * L, L, True)
    mlp(L, O, False)
    return np.concatenate(parts)


def load(quantities, dims, e_norms, n_norms, o_norms, outputs, mps, layer_size, hidden_layers, opt, device, path, index_base=0,
         hip_device=-1, seed=None, gpus=None):
    """`load(...) -> (mgn, opt_state, df_train, df_valid)` with the twelve positional arguments of the reference's call sites
    (src/MeshGraphNets.jl:282-285, 537-540).  With a checkpoint written by `save` in `path`, ALL of its state comes back: parameters,
    loss log, the normalisers' statistics restored over the freshly built `e_norms` / `n_norms` / `o_norms` (what `eval_network`
    relies on, :529-540) and `opt_state` (kept on resume, :287-289; None without a checkpoint or when `opt` is None).  `device` (the
    reference's Lux device function) is accepted and ignored.  gpus (or MGN_GPUS, a comma list, for the unchanged twelve-positional
    call): one partition per listed HIP ordinal behind the same `mgn` (GraphNetwork)."""
    from . import checkpoint as ck
    probe = _capi.load().mgn_param_count
    cfg = MgnConfig(Fn=quantities, Fe=dims + 1, O=outputs, L=layer_size, hidden_layers=hidden_layers, mps=mps, n_edge_sets=1)
    nparams = int(probe(C.byref(cfg)))
    got = ck.read_checkpoint(path, nparams, e_norms, n_norms, o_norms, want_opt_state=opt is not None)
    if got is None:
        ps, opt_state, df_train, df_valid = init_params((quantities, dims + 1, outputs, layer_size, hidden_layers, mps), seed), None, ck.LossLog(), ck.LossLog()
    else:
        ps, e_norms, n_norms, o_norms, opt_state, df_train, df_valid = got
    mgn = GraphNetwork(quantities, dims, e_norms, n_norms, o_norms, outputs, mps, layer_size, hidden_layers, ps=ps,
                       index_base=index_base, device=hip_device, gpus=gpus)
    return mgn, opt_state, df_train, df_valid


def save(mgn, opt_state, df_train, df_valid, step, loss, path, is_training=True):
    """`save!(mgn, opt_state, df_train, df_valid, step, loss, path; is_training)` (src/MeshGraphNets.jl:460-471): appends (step, loss)
    to the training or validation log and writes parameters, normalisers (with whatever an online one has accumulated), optimiser
    state and the log."""
    from . import checkpoint as ck
    log = df_train if is_training else df_valid
    log.step.append(int(step))
    log.loss.append(np.float32(loss))
    ck.write_checkpoint(path, mgn.ps, mgn.e_norm, mgn.n_norm, mgn.o_norm, opt_state, df_train, df_valid)


def step(mgn, graph, target, mask, loss_function=None):
    """GraphNetCore.step!(mgn, graph, target, mask, loss_function) as the reference calls it (src/strategies.jl:418-422):
    returns (gs, loss) with loss = mean(mse_reduce(target, mgn.model(graph))[mask]) and gs = d loss / d mgn.ps in packed
    order, ready for the optimiser update at src/MeshGraphNets.jl:375-377.  `mask` follows mgn.index_base (1-based Int32 node
    indices at the Julia boundary).  Only the reference's loss (mse_reduce) exists on the device: any other callable
    is refused rather than silently replaced."""
    if loss_function is not None and getattr(loss_function, "__name__", "") != "mse_reduce":
        raise ValueError("step: only mse_reduce is implemented on the device (reference src/strategies.jl:421)")
    mgn._sync_params(mgn.ps)
    mgn._sync_graph(graph.senders, graph.receivers, graph.nf.shape[0])
    return mgn.engine.step(graph.nf, graph.ef, target, mask, mask_index_base=mgn.index_base)


# ==================================================================================================
# staged driver shared by the single-GPU loopback test, the RCCL path and the gloo CPU test
# ==================================================================================================
def run_processor_staged(engines, exchange, nsteps, begin=True, overlap=None):
    """engines: objects with proc_begin/proc_edge/proc_node (one per local partition);
    exchange(): performs pack -> all-to-all-v -> unpack for all of them.
    Mirrors mgn_processor_steps_dev for nranks > 1.

    overlap (default: on when the engines and the exchange support it): owned nodes are numbered boundary-first,
    so the projection of the boundary tiles runs first, the exchange is started (exchange.start(): pack + async
    all-to-all-v) and the interior tiles are projected while the rows are on the wire; the next edge step then runs
    its interior tiles (no halo sender) first and only its few boundary tiles after exchange.finish()."""
    if nsteps <= 0:
        return
    if overlap is None:
        overlap = all(hasattr(e, "proc_node_phase") for e in engines) and hasattr(exchange, "start")

    edge_split = overlap and all(hasattr(e, "proc_edge_phase") for e in engines)

    def project_and_start(k):           # k = -1: projection for step 0 (proc_begin); leaves the exchange in flight
        if overlap:
            for e in engines:
                e.proc_node_phase(k, 1)
            exchange.start()
            for e in engines:
                e.proc_node_phase(k, 2)
        else:
            for e in engines:
                e.proc_begin() if k < 0 else e.proc_node(k, True)
            exchange.start() if hasattr(exchange, "start") else exchange()

    def finish():
        if hasattr(exchange, "finish"):
            exchange.finish()

    if begin:
        project_and_start(-1)
    else:
        exchange.start() if hasattr(exchange, "start") else exchange()
    for k in range(nsteps):
        if edge_split:
            # edges whose sender is owned run while the halo rows are on the wire; the few boundary tiles after them
            for e in engines:
                e.proc_edge_phase(k, 1)
            finish()
            for e in engines:
                e.proc_edge_phase(k, 2)
        else:
            finish()
            for e in engines:
                e.proc_edge(k)
        if k + 1 < nsteps:
            project_and_start(k)
        else:
            for e in engines:
                e.proc_node(k, False)


def run_forward_staged(engines, exchange, mps):
    for e in engines:
        e.fwd_encode()
    run_processor_staged(engines, exchange, mps, begin=False)
    for e in engines:
        e.fwd_decode()
