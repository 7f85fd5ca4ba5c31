"""Host-side mirror of the reference functions on either side of the hot path, with the reference's names.

In the real drop-in these stay Julia and unchanged (reference src/graph.jl, src/solve.jl call into
GraphNetCore; only GraphNetCore is replaced).  Julia is not available in this environment, so the same
functions are written here in NumPy float32 to drive the engine exactly the way the reference does:

    create_base_graph      reference src/graph.jl:25-55
    build_graph            reference src/graph.jl:75-97
    ode_func_eval          reference src/solve.jl:147-158
    ode_step               reference src/solve.jl:188-219
    rollout (Euler branch) reference src/solve.jl:42-68  (`solve(prob, solver; adaptive=false, dt, saveat)`)
    train_step (solver strategies with Euler() / Tsit5())  reference src/strategies.jl:175-196, 238-383 (Engine.solver_grad /
                           Engine.solver_grad_tsit5 per solved window)
    init_train_step_derivative  reference src/strategies.jl:395-416 (Engine.step_datapoint is its device form plus step!)
    validation_step, rollout_errors  reference src/strategies.jl:111-134, src/MeshGraphNets.jl:609-628 (Engine.rollout_eval)
    GraphNetCore surface   one_hot, triangles_to_edges, parse_edges, mse_reduce, NormaliserOfflineMinMax,
                           NormaliserOfflineMeanStd, NormaliserOnline, inverse_data (docs/src/graph_net_core.md)

Arrays are [count][feat] (the bytes of Julia's feat x count).  Indices returned by triangles_to_edges /
parse_edges are 0-based here; GraphNetwork(index_base=...) tells the engine which base the caller uses.
"""
from __future__ import annotations

import os

import numpy as np

from . import _capi
from .engine import FeatureGraph

F32 = np.float32


# ---- GraphNetCore utilities ---------------------------------------------------------------------
def one_hot(v, depth, offset=0):
    """one_hot(vec(node_type), type_max - type_min + 1, 1 - type_min) at src/graph.jl:26-27 (the Julia offset
    is 1-based; here offset = -type_min)."""
    v = np.asarray(v).reshape(-1).astype(np.int64) + offset
    if v.size and (v.min() < 0 or v.max() >= depth):
        raise ValueError("ArgumentError: one_hot index outside [0, depth)")
    out = np.zeros((v.size, depth), F32)
    out[np.arange(v.size), v] = 1.0
    return out


def triangles_to_edges(cells):
    """Two-way unique edges of a triangulation in first-occurrence order (src/graph.jl:30)."""
    cells = np.asarray(cells, dtype=np.int64)
    if cells.ndim != 2 or cells.shape[1] != 3:
        raise ValueError("DimensionMismatch: cells must be [C][3]")
    e = np.concatenate([cells[:, 0:2], cells[:, 1:3], cells[:, [2, 0]]], 0)
    hi, lo = e.max(1), e.min(1)
    key = hi * (int(e.max()) + 1) + lo
    _, first = np.unique(key, return_index=True)
    first.sort()
    a, b = hi[first].astype(np.int32), lo[first].astype(np.int32)
    return np.concatenate([a, b]), np.concatenate([b, a])


def parse_edges(edges):
    """parse_edges(data["edges"]) at src/graph.jl:38: explicit [n][2] edge list -> two-way senders/receivers."""
    e = np.asarray(edges, dtype=np.int32)
    if e.ndim != 2 or e.shape[1] != 2:
        raise ValueError("DimensionMismatch: edges must be [n][2]")
    return np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]])


def mse_reduce(target, output):
    """Sum of squared errors over the feature rows, per node (loss_fn of step!, src/strategies.jl:421)."""
    return ((np.asarray(target, F32) - np.asarray(output, F32)) ** 2).sum(-1)


# ---- normalisers (constructed at src/MeshGraphNets.jl:79-203) --------------------------------------
class NormaliserOfflineMinMax:
    def __init__(self, data_min, data_max, target_min=0.0, target_max=1.0):
        self.data_min, self.data_max = F32(data_min), F32(data_max)
        self.target_min, self.target_max = F32(target_min), F32(target_max)

    def __call__(self, x):
        x = np.asarray(x, F32)
        return (x - self.data_min) / (self.data_max - self.data_min) * (self.target_max - self.target_min) + self.target_min

    def inverse(self, y):
        y = np.asarray(y, F32)
        return (y - self.target_min) / (self.target_max - self.target_min) * (self.data_max - self.data_min) + self.data_min

    def affine(self, dim):
        s = (self.target_max - self.target_min) / (self.data_max - self.data_min)
        return np.full(dim, s, F32), np.full(dim, self.target_min - self.data_min * s, F32)

    def inverse_affine(self, dim):
        s = (self.data_max - self.data_min) / (self.target_max - self.target_min)
        return np.full(dim, s, F32), np.full(dim, self.data_min - self.target_min * s, F32)


class NormaliserOfflineMeanStd:
    def __init__(self, mean, std):
        self.mean = np.asarray(mean, F32)
        self.std = np.maximum(np.asarray(std, F32), F32(1e-8))

    def __call__(self, x):
        return (np.asarray(x, F32) - self.mean) / self.std

    def inverse(self, y):
        return np.asarray(y, F32) * self.std + self.mean

    def affine(self, dim):
        s = np.broadcast_to(F32(1.0) / self.std, (dim,)).astype(F32)
        return s, (-np.broadcast_to(self.mean, (dim,)) * s).astype(F32)

    def inverse_affine(self, dim):
        return np.broadcast_to(self.std, (dim,)).astype(F32), np.broadcast_to(self.mean, (dim,)).astype(F32)


class NormaliserOnline:
    """NormaliserOnline(dims, device; max_acc): accumulates sum / sum of squares / count over the rows it is
    called with until max_acc calls, then normalises with the running mean / max(std, 1e-8)."""

    def __init__(self, dims, device=None, max_acc=1e6, std_epsilon=1e-8):
        self.dims, self.max_acc, self.std_epsilon = int(dims), float(max_acc), F32(std_epsilon)
        self.acc_sum = np.zeros(self.dims, np.float64)
        self.acc_sum_squared = np.zeros(self.dims, np.float64)
        self.acc_count = 0.0
        self.num_accumulations = 0.0
        self.engine = None               # set to an Engine to accumulate on the device

    def _accumulate(self, x):
        if self.num_accumulations < self.max_acc:
            if self.engine is not None:          # device reduction (mgn_feature_stats), same float64 totals
                s, q = self.engine.feature_stats(np.ascontiguousarray(x, dtype=np.float32))
                self.acc_sum += s
                self.acc_sum_squared += q
            else:
                self.acc_sum += x.sum(0, dtype=np.float64)
                self.acc_sum_squared += (x.astype(np.float64) ** 2).sum(0)
            self.acc_count += x.shape[0]
            self.num_accumulations += 1.0

    def frozen(self):
        c = max(self.acc_count, 1.0)
        mean = self.acc_sum / c
        std = np.sqrt(np.maximum(self.acc_sum_squared / c - mean * mean, 0.0))
        return NormaliserOfflineMeanStd(mean.astype(F32), np.maximum(std, self.std_epsilon).astype(F32))

    def __call__(self, x, accumulate=True):
        x = np.asarray(x, F32)
        if x.shape[-1] != self.dims:
            raise ValueError("DimensionMismatch: NormaliserOnline built for %d features, got %d" % (self.dims, x.shape[-1]))
        if accumulate:
            self._accumulate(x)
        return self.frozen()(x)

    def inverse(self, y):
        return self.frozen().inverse(y)

    def affine(self, dim):
        return self.frozen().affine(dim)

    def inverse_affine(self, dim):
        return self.frozen().inverse_affine(dim)


def inverse_data(norm, y):
    """inverse_data(mgn.o_norm[field], output_rows) at src/solve.jl:207."""
    return norm.inverse(y)


# ---- src/graph.jl ------------------------------------------------------------------------------------
def create_base_graph(data, type_size, type_min, device=None):
    """Static part of the graph, once per trajectory.  data: dict with 'node_type' [N] (or [N][1]), 'mesh_pos'
    [N][dims] and 'cells' [C][3] or 'edges' [n][2] (either index base, told apart as the reference does: by the presence of a 0).
    Per-node arrays may carry a leading time axis ([T][N][..], what the dataset readers return): the first frame is taken, like
    `data[...][:, :, 1]`.  Returns (node_type_onehot, senders, receivers, edge_features) like src/graph.jl:54 (0-based indices)."""
    first = lambda a, nd: np.asarray(a)[0] if np.asarray(a).ndim > nd else np.asarray(a)     # noqa: E731  ([T][N][..] -> frame 1)
    nt = np.asarray(data["node_type"])
    nt = nt[0] if nt.ndim == 3 else nt
    node_type = one_hot(nt.reshape(-1), type_size - type_min + 1, -type_min)
    if "cells" in data:
        senders, receivers = triangles_to_edges(first(data["cells"], 2))
    elif "edges" in data:
        senders, receivers = parse_edges(data["edges"])
    else:
        raise KeyError("Data does not contain cell or edge information!")
    # src/graph.jl:31-34, 39-42: lists that name a node 0 are 0-based and shifted to Julia's 1-based indices, all others are taken as 1-based
    # already (the HDF5 arm's create_edges / read_edges produce those).  This module indexes from 0: the mirror image of that rule.
    if senders.size and not ((senders == 0).any() or (receivers == 0).any()):
        senders, receivers = senders - 1, receivers - 1
    pos = np.asarray(first(data["mesh_pos"], 2), F32)
    rel = pos[senders] - pos[receivers]
    edge_features = np.concatenate([rel, np.linalg.norm(rel, axis=1, keepdims=True).astype(F32)], 1).astype(F32)
    return node_type, senders, receivers, edge_features


def build_graph(mgn, data, fields, datapoint, node_type, edge_features, senders, receivers):
    """nf = [n_norm[field](data[field]) for field in fields ..., n_norm['node_type'](node_type)]; ef = e_norm(...)
    (src/graph.jl:80-96).  data[field]: [N][dim] or [T][N][dim] (then row min(T, datapoint) is used)."""
    if np.asarray(edge_features).dtype != np.float32:
        raise TypeError("MethodError: edge_features must be Float32 (src/graph.jl:76)")
    cols = []
    for field in fields:
        d = np.asarray(data[field], F32)
        if d.ndim == 3:
            d = d[min(d.shape[0] - 1, datapoint)]
        cols.append(mgn.n_norm[field](d))
    cols.append(mgn.n_norm["node_type"](node_type))
    return FeatureGraph(np.concatenate(cols, 1).astype(F32), mgn.e_norm(edge_features).astype(F32), senders, receivers)


# ---- src/strategies.jl (derivative strategies) ---------------------------------------------------------
def init_train_step_derivative(mgn, data, meta, fields, target_fields, node_type, edge_features, senders, receivers, datapoint):
    """init_train_step(::DerivativeStrategy, ...) at src/strategies.jl:395-416: the normalised change of the target fields over
    one step, then build_graph.  data[field] and data['target|' + field]: [T-1][N][dim] as add_targets! leaves them
    (src/dataset.jl:461-481: the field without its last frame, the target without its first); meta['dt']: a scalar, or an array of
    times, of which the step from `datapoint` to `datapoint + 1` is taken.  datapoint is 0-based here.  Float32 throughout, one
    rounding per operation; the normalisers are called as the reference calls them (an online one accumulates, then normalises).
    Returns (graph, target_quantities_change [N][sum of dims]); Engine.step_datapoint is the device form of this plus step!."""
    dt = meta["dt"]
    if np.ndim(dt) > 0:
        tm = np.asarray(dt, F32)
        delta = F32(tm[datapoint + 1] - tm[datapoint])
    else:
        delta = F32(dt)
    cols = []
    for field in target_fields:
        nxt = np.asarray(data["target|" + field], F32)[datapoint]
        cur = np.asarray(data[field], F32)[datapoint]
        cols.append(np.asarray(mgn.o_norm[field](((nxt - cur) / delta).astype(F32)), F32))
    graph = build_graph(mgn, data, fields, datapoint, node_type, edge_features, senders, receivers)
    return graph, np.concatenate(cols, 1).astype(F32)


# ---- src/solve.jl ------------------------------------------------------------------------------------
def ode_step(x, p, t):
    """x: [N][sum(dims)] state; p = (mgn, ps, inputs, fields, meta, target_fields, target_dict, node_type,
    edge_features, senders, receivers, val_mask, pr) exactly as src/solve.jl:188-191."""
    (mgn, ps, inputs, fields, meta, target_fields, target_dict, node_type, edge_features, senders, receivers,
     val_mask, pr) = p
    offset = 0
    for k in target_fields:
        inputs[k] = x[:, offset:offset + target_dict[k]]
        offset += target_dict[k]
    graph = build_graph(mgn, inputs, fields, 0, node_type, edge_features, senders, receivers)
    output, st = mgn.model(graph, ps, mgn.st)
    mgn.st = st
    indices = [meta["features"][tf]["dim"] for tf in target_fields]
    buf = np.empty_like(output)
    o = 0
    for i, tf in enumerate(target_fields):
        buf[:, o:o + indices[i]] = inverse_data(mgn.o_norm[tf], output[:, o:o + indices[i]])
        o += indices[i]
    return buf * val_mask


def ode_func_eval(x, p, t):
    """Inflow overwrite then ode_step (src/solve.jl:147-158).  p as in the reference plus (data, inflow_mask,
    saves_dt): x[inflow_mask] = vcat(data[field][floor(t / saves_dt)] ...)[inflow_mask]."""
    (mgn, ps, data, inputs, fields, meta, target_fields, target_dict, node_type, edge_features, senders, receivers,
     val_mask, inflow_mask, saves_dt, pr) = p
    # floor(Int, t / saves_dt) + 1 (1-based) in the type t and saves_dt arrive in, no tolerance (src/solve.jl:151): an IndexError
    # here is the reference's BoundsError
    k = int(np.floor(t / saves_dt))
    gt = np.concatenate([np.asarray(data[f], F32)[k] for f in target_fields], 1)
    x[inflow_mask] = gt[inflow_mask]   # IN PLACE, like the reference: the caller's (solver's) state is modified
    return ode_step(x, (mgn, ps, inputs, fields, meta, target_fields, target_dict, node_type, edge_features,
                        senders, receivers, val_mask, pr), t)


def rollout(solver, mgn, initial_state, fields, meta, target_fields, target_dict, node_type, edge_features, senders,
            receivers, val_mask, inflow_mask, data, start, stop, dt, saves, show_progress=False):
    """Fixed-step branch of rollout (src/solve.jl:57-61, `adaptive = false, dt = dt`); solver must be "Euler".
    Returns (sol_u [len(saves)][N][O], sol_t)."""
    if solver != "Euler" or dt is None:
        raise NotImplementedError("only the fixed-step Euler branch is mirrored; adaptive Tsit5 stays in DifferentialEquations.jl")
    x = np.concatenate([np.asarray(initial_state[f], F32) for f in target_fields], 1)
    inputs = {k: v for k, v in initial_state.items() if k not in target_dict}
    p = (mgn, mgn.ps, data, inputs, fields, meta, target_fields, target_dict, node_type, edge_features, senders,
         receivers, val_mask, inflow_mask, saves[1] - saves[0], None)
    sol_u, sol_t = [], []
    t = start
    nsteps = int(round((stop - start) / dt))
    save_set = {int(round((s - start) / dt)) for s in saves}
    for i in range(nsteps + 1):
        if i in save_set:
            sol_u.append(x.copy())
            sol_t.append(t)
        if i == nsteps:
            break
        dx = ode_func_eval(x, p, t)   # mutates the inflow rows of x (reference quirk, src/solve.jl:151-152)
        x = x + F32(dt) * dx
        t = t + dt                    # the integrator's own time: t <- t + dt in the type start / dt arrive in (np.float32 or float)
    return np.stack(sol_u), np.array(sol_t)


# ---- dataset formats -------------------------------------------------------------------------------
class TFRecordReader:
    """Iterator over the tf.train.Example records of a .tfrecord file (native reader: mgn_tfrecord_*), the stand-in for
    TFRecord.jl's `read(path; channel_size)` (reference src/dataset.jl:107-112).  Yields {feature name: (kind, bytes)}
    with kind 1 = bytes_list (first value), 2 = float_list, 3 = int64_list."""

    def __init__(self, path, verify_crc=True):
        import ctypes as C
        from . import _capi
        self._C, self.lib = C, _capi.load()
        self.h = C.c_void_p()
        if self.lib.mgn_tfrecord_open(str(path).encode(), 1 if verify_crc else 0, C.byref(self.h)) != 0:
            raise FileNotFoundError(path)

    def __iter__(self):
        return self

    def __next__(self):
        C = self._C
        rc = self.lib.mgn_tfrecord_next(self.h)
        if rc == 0:
            raise StopIteration
        if rc < 0:
            raise ValueError("ArgumentError: " + self.lib.mgn_tfrecord_error(self.h).decode())
        out = {}
        for i in range(self.lib.mgn_tfrecord_feature_count(self.h)):
            name = self.lib.mgn_tfrecord_feature_name(self.h, i)
            kind, ptr, nb = C.c_int32(), C.c_void_p(), C.c_int64()
            self.lib.mgn_tfrecord_feature(self.h, name, C.byref(kind), C.byref(ptr), C.byref(nb))
            out[name.decode()] = (kind.value, C.string_at(ptr, nb.value) if nb.value else b"")
        return out

    def close(self):
        if self.h:
            self.lib.mgn_tfrecord_close(self.h)
            self.h = self._C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def parse_data(example, meta):
    """parse_data(data::Example, meta) (reference src/dataset.jl:61-75): every feature listed in meta["features"] is
    reinterpreted by its dtype and reshaped to reverse(shape) (a -1 entry resolved from the payload length); static
    features are repeated over the trajectory.  Arrays come back as [T][count][dim] (the bytes of Julia's dim x count x T).
    A feature missing from the record raises KeyError, like `data.features.feature[key]`."""
    out = {}
    for key, value in meta["features"].items():
        kind, payload = example[key]
        d = np.frombuffer(payload, dtype=np.dtype(value["dtype"]))
        shape = list(value["shape"])
        if -1 in shape:
            q = d.size
            for sdim in shape:                      # abs(reduce(div, shape; init = length(d)))
                q = int(q / sdim) if sdim else q    # Julia `div` truncates toward zero
            shape[shape.index(-1)] = abs(q)
        d = d.reshape(shape)
        if value["type"] == "static":
            d = np.repeat(d, meta["trajectory_length"], axis=0)
        out[key] = d
    return out


class Dataset:
    """Dataset (reference src/dataset.jl:36-47): file, file_valid, meta, ch, ch_valid.  `ch` / `ch_valid` are iterators standing in for
    the Channels; unpacking gives (meta, ch), the pair the TFRecord-only version of load_dataset returned."""

    def __init__(self, file, file_valid, meta, ch, ch_valid):
        self.file, self.file_valid, self.meta, self.ch, self.ch_valid = file, file_valid, meta, ch, ch_valid

    def __iter__(self):
        return iter((self.meta, self.ch))


def load_dataset(path, is_training):
    """load_dataset(path, is_training) (reference src/dataset.jl:89-172): `train` or `test` + `.tfrecord`, else `.jld2`, else `.h5`,
    in that order of preference; training also opens the `valid` file of the same format.  The TFRecord arm yields parsed trajectories
    (parse_data), the HDF5 / JLD2 arm the dictionaries of read_h5! (`dataset_h5.read_trajectory`; needs libhdf5, `hdf5_lite`)."""
    import json
    import os
    filename = "train" if is_training else "test"
    if os.path.isfile(os.path.join(path, filename + ".tfrecord")):
        with open(os.path.join(path, "meta.json")) as f:
            meta = json.load(f)
        file, valid = os.path.join(path, filename + ".tfrecord"), os.path.join(path, "valid.tfrecord")

        def records(f):                       # opened when first taken from, like the task behind TFRecord.jl's Channel
            for ex in TFRecordReader(f):
                yield parse_data(ex, meta)
        return Dataset(file, valid, meta, records(file), records(valid) if is_training else None)
    file = filename + (".jld2" if os.path.isfile(os.path.join(path, filename + ".jld2")) else ".h5")
    if not os.path.isfile(os.path.join(path, file)):
        raise FileNotFoundError(f"ArgumentError: {path} does not contain a {filename}.tfrecord or a {filename}.h5 file")
    from . import dataset_h5
    meta, ch, ch_valid = dataset_h5.load_dataset_h5(path, is_training, file)
    return Dataset(os.path.join(path, file), os.path.join(path, "valid" + os.path.splitext(file)[1]), meta, ch, ch_valid)


# ---- trajectory preparation (host side of SURVEY.md N3 / N4; arrays are [T][count][dim] like parse_data's) -------------
def dump_rollout(dump_dir, ti, mesh_pos, gt, prediction, error, timesteps, cells=None):
    """The evaluation output of one trajectory (reference src/MeshGraphNets.jl:630-637: traj_ops / errors / timesteps / cells of
    eval_network!) as a raw dump that julia/write_trajectories.jl turns into the reference's `trajectories.h5`
    (`/<ti>/<name>/{data,size}`, src/MeshGraphNets.jl:638-669) -- for hosts without libhdf5; with it, `dataset_h5.write_trajectories_h5`
    writes the file directly.
    Arrays arrive in this module's [time][count][feat] / [count][feat] order and are written as the bytes of the Julia arrays
    (feat x count x time: the same bytes); `size` is the Julia size.  ti is 1-based like the reference's trajectory counter."""
    import json
    d = os.path.join(str(dump_dir), str(int(ti)))
    os.makedirs(d, exist_ok=True)
    manifest = {}
    items = {"mesh_pos": (mesh_pos, F32), "gt": (gt, F32), "prediction": (prediction, F32), "error": (error, F32), "timesteps": (timesteps, F32)}
    if cells is not None:
        items["cells"] = (cells, np.int32)
    for name, (arr, dt) in items.items():
        a = np.ascontiguousarray(arr, dtype=dt)
        a.tofile(os.path.join(d, name + ".bin"))
        manifest[name] = {"dtype": "Int32" if dt is np.int32 else "Float32", "size": list(reversed(a.shape))}
    with open(os.path.join(d, "manifest.json"), "w") as f:
        json.dump(manifest, f)
    return d


def solver_training_euler(rhs, vjp, x0, gt, dt, val_mask, n_scale):
    """What train_step(::SolverStrategy) computes for SolverTraining with a fixed-step Euler solver (reference
    src/strategies.jl:175-196, 257-292), written as the discrete adjoint the sensitivity algorithm evaluates through VJPs of
    the right-hand side:
        x_{k+1} = x_k + dt f(x_k),   loss = mean(((n_norm(gt_k) - n_norm(x_k)) ^ 2) .* val_mask)  over k = 0..K, nodes, fields
        a_K = dL/dx_K;   a_k = dL/dx_k + a_{k+1} + dt J_x(x_k)^T a_{k+1};   gs = sum_k dt J_p(x_k)^T a_{k+1}
    rhs(x) -> f(x) [N][O];  vjp(x, lam) -> (lam^T df/dx, lam^T df/dps)  (Engine.ode_step / Engine.ode_vjp with the static
    inputs bound);  gt [K+1][N][O];  n_scale [O]: scale of the field normaliser (its shift cancels in the difference).
    Returns (gs, loss, xs)."""
    gt = np.asarray(gt, np.float64)
    K = gt.shape[0] - 1
    vm = np.asarray(val_mask, np.float64).reshape(-1, 1)
    sc = np.asarray(n_scale, np.float64).reshape(1, -1)
    xs = [np.asarray(x0, np.float64)]
    for _ in range(K):
        xs.append(xs[-1] + dt * np.asarray(rhs(xs[-1].astype(F32)), np.float64))
    count = float((K + 1) * gt.shape[1] * gt.shape[2])
    loss = float(sum((((gt[k] - xs[k]) * sc) ** 2 * vm).sum() for k in range(K + 1)) / count)

    def dl_dx(k):
        return -2.0 * sc * sc * (gt[k] - xs[k]) * vm / count

    a = dl_dx(K)
    gs = None
    for k in range(K - 1, -1, -1):
        xbar, g = vjp(xs[k].astype(F32), (dt * a).astype(F32))
        gs = np.asarray(g, np.float64) if gs is None else gs + g
        a = dl_dx(k) + a + np.asarray(xbar, np.float64)
    return gs, loss, xs


# Tsitouras 5(4) (the method OrdinaryDiffEq.jl calls Tsit5): TSIT5_A[i][j] is A[i + 1][j + 1] of the 1-based tableau, row 6 is b
TSIT5_C = (0.0, 0.161, 0.327, 0.9, 0.9800255409045097, 1.0, 1.0)
TSIT5_A = ((0, 0, 0, 0, 0, 0),
           (0.161, 0, 0, 0, 0, 0),
           (-0.008480655492356989, 0.335480655492357, 0, 0, 0, 0),
           (2.8971530571054935, -6.359448489975075, 4.3622954328695815, 0, 0, 0),
           (5.325864828439257, -11.748883564062828, 7.4955393428898365, -0.09249506636175525, 0, 0),
           (5.86145544294642, -12.92096931784711, 8.159367898576159, -0.071584973281401, -0.028269050394068383, 0),
           (0.09646076681806523, 0.01, 0.4798896504144996, 1.379008574103742, -3.290069515436081, 2.324710524099774))
# Tsit5's dense output (the free 4th-order interpolant of Tsitouras 2011, as OrdinaryDiffEq.jl's): x(t_n + theta h) = x_n + h sum_i
# b_i(theta) k_i over the seven stages (k_7 = f(x_{n+1})), b_i(theta) = sum_p TSIT5_R[i][p] theta^(p + 1).  The library's own copy is
# behind mgn_tsit5_interp_weights.
TSIT5_R = ((1.0, -2.763706197274826, 2.9132554618219126, -1.0530884977290216),
           (0.0, 0.13169999999999998, -0.2234, 0.1017),
           (0.0, 3.9302962368947516, -5.941033872131505, 2.490627285651253),
           (0.0, -12.411077166933676, 30.33818863028232, -16.548102889244902),
           (0.0, 37.50931341651104, -88.1789048947664, 47.37952196281928),
           (0.0, -27.896526289197286, 65.09189467479366, -34.87065786149661),
           (0.0, 1.5, -4.0, 2.5))


def solver_training_tsit5(rhs, vjp, x0, gt, step_t, step_h, val_mask=None, n_scale=None, save_step=None, cont_target=None,
                          cont_weight=0.0):
    """The twin of solver_training_euler for Tsit5 over a GIVEN accepted step sequence (step_t, step_h: e.g. what
    Engine.solver_grad_tsit5 recorded), written as the discrete adjoint with the steps held fixed, through VJPs of the right-hand side:
        z_{n,i} = x_n + h_n sum_{j<i} A[i][j] k_{n,j},  k_{n,i} = f(z_{n,i}),  x_{n+1} = x_n + h_n sum_i b_i k_{n,i}
        lam_K = dL/dx_K;  for i = 6 .. 1: kbar_i = h_n (b_i lam + sum_{j>i} A[j][i] zbar_j), (zbar_i, g_i) = vjp(z_{n,i}, kbar_i),
        gs += g_i;  lam_n = lam_{n+1} + sum_i zbar_i + dL/dx_n
    loss = sum_s ((n_scale (gt_s - x_{save_step[s]}))^2 val_mask) / (n_saves N O) + cont_weight sum |x_K - cont_target|.
    rhs(x) -> f(x) [N][O];  vjp(x, lam) -> (lam^T df/dx, lam^T df/dps) (Engine.ode_step / Engine.ode_vjp with the statics bound, no
    inflow);  save_step: the state each save is (default 0 .. K: a save after every step).  The right-hand side has no time here, so
    step_t only has to match step_h in length.  Returns (gs, loss, xs)."""
    A = np.asarray(TSIT5_A, np.float64)
    K = len(step_h)
    if len(step_t) != K:
        raise ValueError("step_t and step_h differ in length")
    gt = np.asarray(gt, np.float64)
    N, O = gt.shape[1], gt.shape[2]
    vm = np.ones((N, 1)) if val_mask is None else np.asarray(val_mask, np.float64).reshape(N, 1)
    sc = np.ones((1, O)) if n_scale is None else np.asarray(n_scale, np.float64).reshape(1, O)
    save_step = list(range(K + 1)) if save_step is None else list(save_step)
    xs, zs = [np.asarray(x0, np.float64)], []
    for n in range(K):
        h, x, k, z = float(step_h[n]), xs[-1], [], []
        for i in range(6):
            zi = x + h * sum(A[i][j] * k[j] for j in range(i)) if i else x.copy()
            z.append(zi)
            k.append(np.asarray(rhs(zi.astype(F32)), np.float64))
        zs.append(z)
        xs.append(x + h * sum(A[6][j] * k[j] for j in range(6)))
    count = float(len(save_step) * N * O)
    loss = float(sum((((gt[s] - xs[k]) * sc) ** 2 * vm).sum() for s, k in enumerate(save_step)) / count)
    ct = None if cont_target is None else np.asarray(cont_target, np.float64)
    if ct is not None:
        loss += float(cont_weight) * float(np.abs(xs[K] - ct).sum())

    def dl_dx(k):
        g = np.zeros((N, O))
        for s, ks in enumerate(save_step):
            if ks == k:
                g += -2.0 * sc * sc * (gt[s] - xs[k]) * vm / count
        if k == K and ct is not None:
            g += float(cont_weight) * np.sign(xs[K] - ct)
        return g

    lam = dl_dx(K)
    gs = None
    for n in range(K - 1, -1, -1):
        h, zbar = float(step_h[n]), [None] * 6
        for i in range(5, -1, -1):
            kbar = h * (A[6][i] * lam + sum(A[j][i] * zbar[j] for j in range(i + 1, 6)))
            xb, g = vjp(zs[n][i].astype(F32), kbar.astype(F32))
            zbar[i] = np.asarray(xb, np.float64)
            gs = np.asarray(g, np.float64).copy() if gs is None else gs + g
        lam = lam + sum(zbar) + dl_dx(n)
    return gs, loss, xs


def _range_length(tstart, dt, tstop):
    """length(tstart:dt:tstop)."""
    return int(np.floor((float(tstop) - float(tstart)) / float(dt) + 1e-4)) + 1


def _range_at(tstart, dt, i, time_type):
    """(tstart:dt:tstop)[i + 1] in the range's element type."""
    return float(np.dtype(time_type).type(float(tstart) + i * float(dt)))


def multiple_shooting_ranges(T, interval_size):
    """The windows of train_loss(::MultipleShooting) (reference src/strategies.jl:336-337),
    `ranges = [i:min(T, i + interval_size - 1) for i in 1:(interval_size - 1):(T - 1)]`, as 0-based inclusive (first, last) pairs:
    consecutive windows share their end point."""
    if interval_size < 2:
        raise ValueError("interval_size must be >= 2")
    return [(i - 1, min(T, i + interval_size - 1) - 1) for i in range(1, T, interval_size - 1)]


def _solver_window(eng, solver, adaptive, abstol, reltol, x0, node_type_onehot, ef_raw, gt, t0, t1, solver_dt, saves_dt, n_saves, **kw):
    """One solved window through Engine.solver_grad (Euler), Engine.solver_grad_tsit5 (Tsit5) or, for another method Engine.rollout
    takes ("RK4", "BS3", ..., an ErkTableau), Engine.solver_grad_erk with fixed steps of solver_dt: (gs, loss)."""
    if isinstance(solver, str) and solver == "Euler":
        return eng.solver_grad(x0, node_type_onehot, ef_raw, gt, t0, t1, solver_dt, saves_dt, n_saves, **kw)
    if not (isinstance(solver, str) and solver == "Tsit5"):
        if isinstance(solver, str) and solver not in _capi.ERK_NAMES:
            raise ValueError(f"solver must be 'Euler', 'Tsit5', another of {sorted(_capi.ERK_NAMES)} or an ErkTableau, got {solver!r}")
        gs, loss, _ = eng.solver_grad_erk(solver, x0, node_type_onehot, ef_raw, gt, t0, t1, saves_dt, n_saves, solver_dt, **kw)
        return gs, loss
    gs, loss, _ = eng.solver_grad_tsit5(x0, node_type_onehot, ef_raw, gt, t0, t1, saves_dt, n_saves, dt=solver_dt or 0.0, adaptive=adaptive,
                                        abstol=abstol, reltol=reltol, **kw)
    return gs, loss


def train_step_solver_training(eng, gt, node_type_onehot, ef_raw, tstart, dt, tstop, val_mask=None, inflow_mask=None, inflow_data=None,
                               n_scale=None, solver_dt=None, time_type=F32, inflow_rule="reference", out=None, solver="Euler",
                               adaptive=True, abstol=1e-6, reltol=1e-3):
    """train_step(::SolverTraining) with a fixed-step Euler solver (reference src/strategies.jl:175-196, 257-292) in one native call:
    u0 = gt[1], saveat = tstart:dt:tstop, loss = mean(((n_norm(gt) - n_norm(pred)) .^ 2) .* val_mask).  gt [T][N][O] (the trajectory's
    target fields, T >= the number of save points); n_scale [O]: scale of the field normaliser (its shift cancels); inflow_mask [N]:
    rows overwritten inside the right-hand side from inflow_data [frames][N][O] (default: gt itself, data[field] of ode_func_train,
    src/solve.jl:101-117); solver_dt: the Euler step (default dt, the example's tstops = saveat).  solver="Tsit5":
    Engine.solver_grad_tsit5, adaptive (first step solver_dt, default 0: the Hairer-Wanner start; abstol / reltol) or, with
    adaptive=False, fixed steps of solver_dt (default dt).  solver="RK4", "Heun", "BS3", "DP5", ... or an ErkTableau:
    Engine.solver_grad_erk, fixed steps of solver_dt (default dt) whatever `adaptive` says.  Returns (gs, loss): the discrete adjoint of
    the computed solution (Tsit5: with the accepted steps held fixed)."""
    n_saves = _range_length(tstart, dt, tstop)
    if inflow_mask is not None and inflow_data is None:
        inflow_data = gt
    sdt = solver_dt if (isinstance(solver, str) and solver == "Tsit5" and adaptive) else (solver_dt or dt)
    return _solver_window(eng, solver, adaptive, abstol, reltol, np.asarray(gt[0]), node_type_onehot, ef_raw, gt[:n_saves], tstart, tstop,
                          sdt, dt, n_saves, val_mask=val_mask, inflow_mask=inflow_mask, inflow_data=inflow_data, loss_scale=n_scale,
                          inflow_rule=inflow_rule, time_type=time_type, out=out)


def train_step_multiple_shooting(eng, gt, node_type_onehot, ef_raw, tstart, dt, tstop, interval_size, continuity_term, val_mask=None,
                                 inflow_mask=None, inflow_data=None, solver_dt=None, time_type=F32, inflow_rule="reference", solver="Euler",
                                 adaptive=True, abstol=1e-6, reltol=1e-3, batched=False, max_windows_per_pass=0, interpolate_saves=False):
    """train_step(::MultipleShooting) with a fixed-step Euler solver (reference src/strategies.jl:312-383): one Engine.solver_grad per
    window rg of multiple_shooting_ranges, u0 = gt[first(rg)], saveat = tsteps[rg], loss = mean((gt[rg] - pred) .^ 2 .* val_mask) (no
    normaliser); the continuity term continuity_term * sum(abs, pred_{i-1}[end] - gt[first(rg_i)]) goes with window i - 1.  solver,
    adaptive, abstol, reltol as for train_step_solver_training.  Returns the summed (gs, loss).
    interpolate_saves (solver="Tsit5"): False (the default, the bits this function has always returned) steps every window onto its
    saves, tstops = saveat.  True is what the reference computes: it solves every window with saveat and NO tstops
    (src/strategies.jl:343-355), so the steps end on the window's end only and the saves between them come from Tsit5's dense output
    (Engine.solver_grad_tsit5(dense_saves=True)); per window, not with batched=True.
    batched=True: Euler and fixed-step Tsit5 (adaptive=False) solve all windows in one Engine.shooting_grad call (windows with the same
    step plan as one batch of graph copies, at most max_windows_per_pass per pass, 0: no cap) -- the same sum.  Adaptive Tsit5 keeps the
    per-window loop (each window would need its own step controller)."""
    T = _range_length(tstart, dt, tstop)
    ranges = multiple_shooting_ranges(T, interval_size)
    if inflow_mask is not None and inflow_data is None:
        inflow_data = gt
    if interpolate_saves and solver != "Tsit5":
        raise ValueError("interpolate_saves is Tsit5's dense output: solver must be 'Tsit5'")
    if interpolate_saves and batched:
        raise ValueError("interpolate_saves solves window by window: Engine.shooting_grad steps onto every save (batched must be False)")
    dense = {"dense_saves": True} if interpolate_saves else {}
    if batched and solver not in ("Euler", "Tsit5"):
        raise ValueError("batched=True (Engine.shooting_grad) drives 'Euler' and 'Tsit5'; other methods go window by window")
    if batched and not (solver == "Tsit5" and adaptive):
        gs, loss = eng.shooting_grad(node_type_onehot, ef_raw, gt, ranges, [_range_at(tstart, dt, a, time_type) for a, _ in ranges],
                                     [_range_at(tstart, dt, b, time_type) for _, b in ranges], solver_dt or dt, dt, val_mask=val_mask,
                                     inflow_mask=inflow_mask, inflow_data=inflow_data, cont_weight=float(continuity_term),
                                     inflow_rule=inflow_rule, time_type=time_type, solver=solver, max_windows_per_pass=max_windows_per_pass)
        return np.asarray(gs, np.float64), float(loss)
    gs_sum, loss_sum = None, 0.0
    for i, (a, b) in enumerate(ranges):
        nxt = ranges[i + 1][0] if i + 1 < len(ranges) else None
        sdt = solver_dt if (solver == "Tsit5" and adaptive) else (solver_dt or dt)
        gs, loss = _solver_window(eng, solver, adaptive, abstol, reltol, np.asarray(gt[a]), node_type_onehot, ef_raw, gt[a:b + 1],
                                  _range_at(tstart, dt, a, time_type), _range_at(tstart, dt, b, time_type), sdt, dt, b - a + 1,
                                  val_mask=val_mask, inflow_mask=inflow_mask, inflow_data=inflow_data,
                                  cont_target=None if nxt is None else gt[nxt], cont_weight=float(continuity_term) if nxt is not None else 0.0,
                                  inflow_rule=inflow_rule, time_type=time_type, **dense)
        gs_sum = np.asarray(gs, np.float64) if gs_sum is None else gs_sum + gs
        loss_sum += float(loss)
    return gs_sum, loss_sum


def _fixed_step_kw(fixed_step, solver, step):
    """rollout_eval's extra keywords for the reference's `adaptive = false, dt = dt` branch: Tsit5 -- or any other method Engine.rollout
    takes ("RK4", "BS3", "DP5", ..., an ErkTableau) -- with a step given, when asked for; "Euler" steps that way already"""
    return {"adaptive": False} if (fixed_step and not (isinstance(solver, str) and solver == "Euler") and step) else {}


def validation_step(eng, data_gt, node_type_onehot, ef_raw, sim_interval, mask, solver="Tsit5", solver_dt=None, val_mask=None,
                    inflow_mask=None, mask_index_base=0, time_type=F32, inflow_rule="reference", abstol=1e-6, reltol=1e-3,
                    want_arrays=False, fixed_step=False):
    """_validation_step (reference src/strategies.jl:111-134; every strategy's validation_step) in one native call, Engine.rollout_eval:
    a rollout from data_gt[0] over sim_interval = (tstart, dt, tstop) saved at tstart:dt:tstop, `error = mean((prediction - gt) .^ 2;
    dims = 3)` and `mean(error[mask])` -- reduced on the device, the solution downloaded only with want_arrays.  data_gt [T][N][O]: the
    trajectory's target fields (T >= the number of saves); with an inflow_mask [N] it is the inflow data too, and is uploaded once.
    mask: the reference's vector of node indices (mask_index_base 0, or 1 as in Julia).  Indexing the O x N matrix `error` with it is
    LINEAR indexing: it selects the elements mask[i] of the [N][O] array, not the rows -- reproduced as it is.
    fixed_step: the reference's own branch on dt (src/solve.jl:57-61) is fixed_step=True whenever a step is given -- `solve(prob, solver;
    adaptive = false, dt = dt, saveat = saves)` whatever the solver, which is how _validation_step hands `solver_valid_dt` on.  With
    solver="Tsit5" and a solver_dt it passes adaptive=False (fixed steps of solver_dt, saves from the dense output); "Euler" steps that way
    already.  The default False is kept for the results this function has always returned: adaptive Tsit5 with solver_dt as its first step.
    solver: any `solver` of Engine.rollout ("Heun", "Midpoint", "Ralston", "RK4", "BS3", "DP5", an ErkTableau); fixed_step as for "Tsit5".
    Returns (loss, None, None) or, with want_arrays, (loss, gt [n_saves][N][O], prediction [n_saves][N][O])."""
    tstart, dt, tstop = sim_interval
    n_saves = _range_length(tstart, dt, tstop)
    if data_gt.shape[0] < n_saves:
        raise ValueError(f"BoundsError: {n_saves} saves, {data_gt.shape[0]} ground-truth frames")
    r = eng.rollout_eval(solver, np.asarray(data_gt[0]), node_type_onehot, ef_raw, data_gt, tstart, _range_at(tstart, dt, n_saves - 1, time_type),
                         dt, n_saves, dt=solver_dt or 0.0, val_mask=val_mask, inflow_mask=inflow_mask,
                         inflow_data=data_gt if inflow_mask is not None else None, abstol=abstol, reltol=reltol, inflow_rule=inflow_rule,
                         time_type=time_type, sel=np.asarray(mask, np.int32), sel_index_base=mask_index_base, want_pred=want_arrays,
                         **_fixed_step_kw(fixed_step, solver, solver_dt))
    if not want_arrays:
        return r["val_loss"], None, None
    return r["val_loss"], np.asarray(data_gt[:n_saves]), r["pred"]


def rollout_errors(eng, data_gt, node_type_onehot, ef_raw, start, stop, dt, saves, mse_steps, solver="Tsit5", val_mask=None, inflow_mask=None,
                   time_type=F32, inflow_rule="reference", abstol=1e-6, reltol=1e-3, fixed_step=False):
    """The error table of eval_network! (reference src/MeshGraphNets.jl:609-628) without the solution leaving the device: a rollout
    from data_gt[0] over (start, stop) saved at `saves` (evenly spaced times from `start`), `error = mean((prediction - gt) .^ 2;
    dims = 2)` as Engine.rollout_eval's mse_save, and for every horizon of mse_steps
        mse = mean(error[:, 1, k]),  cum_mse = mean(error[:, 1, 1:k]),  cum_rmse = sqrt(cum_mse),   k = findfirst(==(horizon), saves).
    dt: the fixed solver step, or None (adaptive Tsit5), as eval_network!'s.  fixed_step: the reference's own branch on dt
    (src/solve.jl:57-61) is fixed_step=True whenever a step is given (`adaptive = false, dt = dt` whatever the solver); with solver="Tsit5"
    and a dt it passes adaptive=False.  The default False is kept for the results this function has always returned (adaptive Tsit5
    with dt as its first step).  solver: any `solver` of Engine.rollout, a tableau included; fixed_step as for "Tsit5".
    Returns (error [n_saves][O] float64, {horizon: (mse, cum_mse, cum_rmse)})."""
    saves = np.asarray(saves, dtype=time_type)
    n_saves = int(saves.size)
    saves_dt = float(saves[1] - saves[0]) if n_saves > 1 else float(stop - start) or 1.0
    r = eng.rollout_eval(solver, np.asarray(data_gt[0]), node_type_onehot, ef_raw, data_gt, start, stop, saves_dt, n_saves, dt=dt or 0.0,
                         val_mask=val_mask, inflow_mask=inflow_mask, inflow_data=data_gt if inflow_mask is not None else None,
                         abstol=abstol, reltol=reltol, inflow_rule=inflow_rule, time_type=time_type, **_fixed_step_kw(fixed_step, solver, dt))
    error = r["mse_save"]
    table = {}
    for horizon in mse_steps:
        hit = np.nonzero(saves == np.dtype(time_type).type(horizon))[0]
        if hit.size == 0:
            raise ValueError(f"horizon {horizon} is not a save point")     # (reference: findfirst gives nothing)
        k = int(hit[0])
        cum = float(np.mean(error[:k + 1]))
        table[horizon] = (float(np.mean(error[k])), cum, float(np.sqrt(cum)))
    return error, table
