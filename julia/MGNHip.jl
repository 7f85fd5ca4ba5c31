# MGNHip.jl -- thin `ccall` shim that puts libmgn_hip.so behind the GraphNetCore surface
# una-auxme/MeshGraphNets.jl uses, so that src/graph.jl, src/solve.jl, src/strategies.jl and the update loop of
# src/MeshGraphNets.jl:375-377 keep working unchanged.
#
# NOT EXECUTED IN THIS REPOSITORY'S CI: julia is not available in the build environment.  What CAN be checked without
# Julia is checked: tests/test_julia_shim.py parses every `ccall` below and the two struct mirrors and compares symbol, argument
# count, C types and field order with include/mgn_hip.h.  The Python ctypes host (meshgraphnets.jl_amd/engine.py) mirrors this
# file call for call and is the tested twin.  See INTEGRATION.md for the diff against src/MeshGraphNets.jl.
#
# Usage inside MeshGraphNets.jl:   replace `using GraphNetCore` (src/MeshGraphNets.jl:8) by
#     include("MGNHip.jl"); using .MGNHip
# and nothing else in src/graph.jl / src/solve.jl / src/strategies.jl.  The names GraphNetCore keeps providing (normalisers,
# one_hot, triangles_to_edges, parse_edges, mse_reduce, inverse_data) are imported HERE, selectively, and re-exported: with both
# `using GraphNetCore` and `using .MGNHip` in the host module, `GraphNetwork`, `FeatureGraph`, `step!`, `load` and `save!` would be
# exported twice and `build_graph(mgn::GraphNetwork, ...)` (src/graph.jl:75) could not resolve its own signature.
module MGNHip

import GraphNetCore
import GraphNetCore: one_hot, triangles_to_edges, parse_edges, mse_reduce, inverse_data,
                     NormaliserOffline, NormaliserOfflineMinMax, NormaliserOfflineMeanStd, NormaliserOnline
import ChainRulesCore
import Serialization      # stdlib: normalisers + optimiser state of a checkpoint (load / save!)
import ChainRulesCore: NoTangent, ZeroTangent, Tangent

# what `using GraphNetCore` gave the reference, minus the five names replaced below
export one_hot, triangles_to_edges, parse_edges, mse_reduce, inverse_data
export NormaliserOffline, NormaliserOfflineMinMax, NormaliserOfflineMeanStd, NormaliserOnline
# the replaced surface
export FeatureGraph, GraphNetwork, step!, load, save!, shooting_grad
# engine extras (optional fast paths; none is needed for the drop-in)
export set_trajectory_graph!, pack_params, init_params, set_norms!, freeze_norms!, set_static!, ode_step_resident, ode_step_fused,
       native_rollout, ode_vjp, forward_vjp, feature_stats, solver_grad, solver_grad_tsit5, solver_grad_erk, native_solver_train_step
export rollout_eval, native_validation_step
export train_trajectory!, step_datapoint!, step_datapoints!, online_norms!, norm_state, norm_state!, datapoint_export
export adam_init!, adam_update!, adam_state, adam_state!, set_params_dev!, get_params_dev!, resident_params!
export comm_unique_id, comm_init!, comm_init_file!, comm_barrier, processor_steps_dev!

const LIB = get(ENV, "MGN_HIP_LIB", joinpath(@__DIR__, "..", "meshgraphnets.jl_amd", "lib", "libmgn_hip.so"))
const ABI_VERSION = 4       # MGN_ABI_VERSION of the include/mgn_hip.h the two struct mirrors below were written against

struct MgnConfig            # mirrors `mgn_config` (include/mgn_hip.h), field for field
    Fn::Int32
    Fe::Int32
    O::Int32
    L::Int32
    hidden_layers::Int32
    mps::Int32
    dtype::Int32
    rank::Int32
    nranks::Int32
    device::Int32
    n_edge_sets::Int32      # 1: the reference's single edge set (src/graph.jl:87-96)
    Fe2::Int32
    ln_mode::Int32          # 0: (x - mean) / sqrt(var + eps); 1: (x - mean) / (sqrt(var) + eps) -- see julia/spec_probe.jl
    ln_dims::Int32          # 0: LayerNorm statistics per node / edge; 1: over the whole array (Lux LayerNorm(shape) at dims = Colon())
end

mutable struct MgnRolloutDesc   # mirrors `mgn_rollout_desc` (include/mgn_hip.h), field for field
    solver::Int32
    t0::Float32
    t1::Float32
    dt::Float32
    saves_dt::Float32
    n_saves::Int32
    abstol::Float32
    reltol::Float32
    x0::Ptr{Float32}
    node_type_onehot::Ptr{Float32}
    ef_raw::Ptr{Float32}
    val_mask::Ptr{Float32}
    inflow_mask::Ptr{UInt8}
    inflow_data::Ptr{Float32}
    n_frames::Int32
    out::Ptr{Float32}
    n_accept::Int32
    n_reject::Int32
    n_rhs::Int32
    inflow_rule::Int32
    time_f64::Int32
    t0_f64::Float64
    t1_f64::Float64
    dt_f64::Float64
    saves_dt_f64::Float64
end

mutable struct MgnSolverGradOpts   # mirrors `mgn_solver_grad_opts` (include/mgn_hip.h), field for field
    adaptive::Int32
    step_cap::Int32
    step_t::Ptr{Float64}
    step_h::Ptr{Float64}
    max_store_bytes::Csize_t
    n_steps::Int32
    stored_bytes::Csize_t
end

mutable struct MgnShootingDesc   # mirrors `mgn_shooting_desc` (include/mgn_hip.h), field for field
    n_windows::Int32
    first::Ptr{Int32}
    last::Ptr{Int32}
    t0::Ptr{Float64}
    t1::Ptr{Float64}
    n_gt::Int32
    adaptive::Int32
    max_windows_per_pass::Int32
    max_batch_nodes::Int64
    n_groups::Int32
    n_passes::Int32
end

mutable struct MgnRolloutEvalDesc   # mirrors `mgn_rollout_eval_desc` (include/mgn_hip.h), field for field
    gt::Ptr{Float32}
    n_gt::Int32
    mse_save::Ptr{Float64}
    mse_time::Ptr{Float32}
    sel::Ptr{Int32}
    n_sel::Int64
    sel_index_base::Int32
    val_loss::Float64
end

function check(h::Ptr{Cvoid}, rc::Cint)
    rc == 0 && return
    msg = unsafe_string(ccall((:mgn_last_error, LIB), Cstring, (Ptr{Cvoid},), h))
    rc == -1 ? throw(ArgumentError(msg)) : error("mgn_hip ($rc): $msg")
end

"FeatureGraph(nf, ef, senders, receivers) -- same fields as GraphNetCore's (reference src/graph.jl:87-96)."
struct FeatureGraph{A <: AbstractMatrix{Float32}, B <: AbstractMatrix{Float32}, I <: AbstractVector{<:Integer}}
    nf::A          # (Fn x N)  == row-major [N][Fn]
    ef::B          # (Fe x E)
    senders::I     # 1-based
    receivers::I
end

"""
Mutable holder with the fields the reference reads and writes: `model`, `ps`, `st`, `e_norm`, `n_norm`, `o_norm`
(src/solve.jl:54,200-208; src/graph.jl:80-93; src/MeshGraphNets.jl:288,376-377).  `ps` is ONE packed Vector{Float32} in
MGN-spec order (pack_params): `Optimisers.setup(opt, mgn.ps)` / `Optimisers.update(opt_state, mgn.ps, gs[i])` work on it as on any
array; it is handed to the engine before every call (mgn_set_params recognises unchanged values: sync_params!).
"""
mutable struct GraphNetwork
    handle::Ptr{Cvoid}
    cfg::MgnConfig
    model::Function
    ps
    st
    e_norm
    n_norm
    o_norm
    graph_key::Tuple{Int, Int, UInt, UInt}     # (E, N, hash(senders), hash(receivers)) of the graph the engine holds
    resident::Bool                             # the engine's device copy of the parameters is the authoritative one (adam_init!): `ps` is not handed over before a call
end

# `rank` / `nranks`: this process's partition of an edge-cut mesh (one process per GPU; see comm_init!).  The reference
# itself is single-device (src/MeshGraphNets.jl:255-263).
# `ln_mode`, `ln_dims`: what julia/spec_probe.jl reports for the installed GraphNetCore / Lux (0 unless it says otherwise).
function GraphNetwork(quantities, dims, e_norm, n_norm, o_norm, outputs, mps, layer_size, hidden_layers, ps; device = -1,
        rank = 0, nranks = 1, ln_mode = 0, ln_dims = 0)
    v = ccall((:mgn_abi_version, LIB), Cint, ())
    v == ABI_VERSION || error("libmgn_hip.so has ABI version $v, this shim is written for $ABI_VERSION")
    cfg = MgnConfig(quantities, dims + 1, outputs, layer_size, hidden_layers, mps, 0, rank, nranks, device, 1, 0, ln_mode, ln_dims)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    rc = ccall((:mgn_create, LIB), Cint, (Ref{MgnConfig}, Ref{Ptr{Cvoid}}), cfg, h)
    rc == 0 || error(unsafe_string(ccall((:mgn_last_error, LIB), Cstring, (Ptr{Cvoid},), C_NULL)))
    mgn = GraphNetwork(h[], cfg, identity, ps, NamedTuple(), e_norm, n_norm, o_norm, (-1, -1, UInt(0), UInt(0)), false)
    mgn.model = (graph, ps_, st) -> (forward(mgn, graph, ps_), st)      # mgn.model(graph, ps, st) -> (output, st)
    finalizer(m -> ccall((:mgn_destroy, LIB), Cvoid, (Ptr{Cvoid},), m.handle), mgn)
    return mgn
end

param_count(cfg::MgnConfig) = Int(ccall((:mgn_param_count, LIB), Csize_t, (Ref{MgnConfig},), cfg))

"""
Flatten a Lux parameter tree into MGN-spec packed order (include/mgn_hip.h): enc-node, enc-edge, step1-edge,
step1-node, ..., decoder; per MLP W1,b1,W2,b2,W3,b3,[ln_scale,ln_bias].  A Lux `Dense` weight is (out x in)
column-major, i.e. the row-major [in][out] block the engine expects: `vec(W)` is already the right bytes.
`leaves` must enumerate the (weight, bias, ...) arrays in that order for the concrete GraphNetCore model.
"""
pack_params(leaves) = reduce(vcat, (vec(Float32.(Array(x))) for x in leaves))

"""
Fresh parameters in packed order: Glorot-uniform weights, zero biases, LayerNorm scale 1 / bias 0 (Lux's defaults for `Dense` and
`LayerNorm`, which GraphNetCore's `build_mlp` uses [GNC-unverified]; the draws are Julia's, not GraphNetCore's).
"""
function init_params(cfg::MgnConfig; rng = nothing)
    r = rng === nothing ? () : (rng,)
    L, h = Int(cfg.L), Int(cfg.hidden_layers)
    ps = Float32[]
    function mlp!(fin, fout, ln)
        dims = vcat(fin, fill(L, h), fout)
        for i in 1:(length(dims) - 1)
            a = sqrt(6.0f0 / (dims[i] + dims[i + 1]))
            append!(ps, (rand(r..., Float32, dims[i] * dims[i + 1]) .* 2.0f0 .- 1.0f0) .* a)
            append!(ps, zeros(Float32, dims[i + 1]))
        end
        ln && (append!(ps, ones(Float32, fout)); append!(ps, zeros(Float32, fout)))
    end
    mlp!(Int(cfg.Fn), L, true)
    mlp!(Int(cfg.Fe), L, true)
    for _ in 1:cfg.mps
        mlp!(3L, L, true)
        mlp!(2L, L, true)
    end
    mlp!(L, Int(cfg.O), false)
    @assert length(ps) == param_count(cfg)
    return ps
end

# ---- load / save!: the checkpoint surface of src/MeshGraphNets.jl:282-285,460-471,537-540 ----------------------------------------
# What the unchanged call sites assume of GraphNetCore's pair (and what therefore round-trips here):
#   * `eval_network` builds FRESH normalisers with calc_norms and relies on `load` to bring back the trained ones (:529-540): a
#     cylinder_flow model normalises velocity (in and out) and the edge features with `NormaliserOnline` (:92,193-199), whose
#     statistics exist nowhere but in the training run that accumulated them;
#   * `train_network` resumes with `step = last(df_train.step)` (:324-325), already past `norm_steps`, so online normalisers never
#     re-accumulate, and it keeps the optimiser state `load` returns (:287-289: `Optimisers.setup` only when it is `nothing`).
# Four files in `path`: packed parameters (raw Float32), the loss log (CSV), the normalisers and the optimiser state (Julia's
# Serialization stdlib).  GraphNetCore's own JLD2 checkpoints are NOT read (different parameter tree, and JLD2 is not a dependency of
# this shim): a run started under GraphNetCore is continued by exporting its leaves once with `pack_params`.
"Loss log with the two columns the reference reads (`df_train.step`, `df_valid.loss`, src/MeshGraphNets.jl:324-330,383)."
mutable struct LossLog
    step::Vector{Int}
    loss::Vector{Float32}
end
LossLog() = LossLog(Int[], Float32[])

const CKPT_PARAMS = "mgn_hip_params.f32"      # packed parameters, raw little-endian Float32
const CKPT_LOG = "mgn_hip_log.csv"            # kind,step,loss
const CKPT_NORMS = "mgn_hip_norms.jls"        # snapshot((e_norm, n_norm, o_norm)): plain data, no device arrays, no closures
const CKPT_OPT = "mgn_hip_opt_state.jls"      # the Optimisers.jl state tree of the packed vector (host arrays), as it is
const CKPT_MANIFEST = "mgn_hip_manifest.txt"   # name,size,checksum of the four files above, written last (checkpoint.py's twin)

"""
`snapshot(x)`: a normaliser (or a Dict / tuple of them) as plain data -- arrays as host `Array`s, numbers and strings as they are,
structs as `(type = name, fields = Dict(field => snapshot))`, functions (the Lux device function a `NormaliserOnline` may keep)
dropped.  Written without naming any field of GraphNetCore's types [GNC-unverified]: whatever they hold is what is stored.
"""
snapshot(x::AbstractArray{<:Number}) = Array(x)
snapshot(x::AbstractArray) = map(snapshot, Array(x))
snapshot(x::Union{Number, AbstractString, Symbol, Nothing}) = x
snapshot(x::Function) = nothing
snapshot(x::AbstractDict) = Dict(k => snapshot(v) for (k, v) in x)
snapshot(x::Tuple) = map(snapshot, x)
snapshot(x::NamedTuple) = map(snapshot, x)
function snapshot(x)
    isstructtype(typeof(x)) || return x
    return (type = String(nameof(typeof(x))), fields = Dict(String(f) => snapshot(getfield(x, f)) for f in fieldnames(typeof(x))))
end

"""
`restore(template, snap)`: the stored statistics put over a freshly built normaliser of the same kind (the ones `calc_norms` hands
to `load`); returns the object to use.  Arrays are copied INTO the template's arrays (they stay on whatever device the template put
them: `copyto!` crosses), other fields are set on mutable structs; an immutable struct whose scalars differ is rebuilt through its
default constructor.  A kind mismatch (an online normaliser stored, an offline one passed) is an error, not a silent pick.
"""
restore(t::AbstractArray{<:Number}, s::AbstractArray{<:Number}) =
    size(t) == size(s) ? copyto!(t, s) : copyto!(similar(t, eltype(t), size(s)), s)
restore(t::Function, s) = t
restore(t::AbstractDict, s::AbstractDict) = (for (k, v) in s; t[k] = haskey(t, k) ? restore(t[k], v) : v; end; t)
restore(t::Tuple, s::Tuple) = map(restore, t, s)
function restore(t, s)
    (s isa NamedTuple && haskey(s, :type) && haskey(s, :fields)) || return s          # plain value: the stored one
    String(nameof(typeof(t))) == s.type ||
        throw(ArgumentError("checkpoint holds a $(s.type), load was handed a $(nameof(typeof(t))): build the normalisers as the training run did"))
    names = fieldnames(typeof(t))
    vals = [haskey(s.fields, String(f)) ? restore(getfield(t, f), s.fields[String(f)]) : getfield(t, f) for f in names]
    if ismutable(t)
        for (f, v) in zip(names, vals)
            v === getfield(t, f) || setfield!(t, f, convert(fieldtype(typeof(t), f), v))
        end
        return t
    end
    all(v === getfield(t, f) || v == getfield(t, f) for (f, v) in zip(names, vals)) && return t     # arrays were filled in place
    return typeof(t)(vals...)
end

"""
    load(quantities, dims, e_norms, n_norms, o_norms, outputs, mps, layer_size, hidden_layers, opt, device, path)
        -> (mgn, opt_state, df_train, df_valid)

Same call shape and return shape as GraphNetCore.load at src/MeshGraphNets.jl:282-285 and :537-540, so both call sites stay as they
are.  `device` (the reference's Lux device function) is accepted and ignored: the engine owns its GPU memory.  With a checkpoint
written by `save!` below in `path`, everything `save!` was given comes back: the parameters, the loss log, the NORMALISERS (their
stored statistics restored over `e_norms` / `n_norms` / `o_norms`, which `calc_norms` has just built empty: `eval_network` relies
on this, :529-540) and `opt_state` (so a resumed run keeps its Adam moments; `nothing` only when there is no checkpoint or `opt` is
`nothing`, which :287-289 turns into `Optimisers.setup(opt, mgn.ps)`).  A checkpoint that has parameters but no normaliser file (one
written before this was stored) is refused when any passed normaliser is a `NormaliserOnline`: it would evaluate with empty statistics.
"""
function load(quantities, dims, e_norms, n_norms, o_norms, outputs, mps, layer_size, hidden_layers, opt, device, path;
        hip_device = -1, ln_mode = 0, ln_dims = 0)
    df_train, df_valid = LossLog(), LossLog()
    opt_state = nothing
    pfile = joinpath(path, CKPT_PARAMS)
    have = isfile(pfile)
    if have
        mfile = joinpath(path, CKPT_MANIFEST)
        if isfile(mfile)               # (absent: a checkpoint written before the manifest existed -- taken as it is)
            for line in eachline(mfile)
                name, size, chk = split(line, ',')
                f = joinpath(path, name)
                (isfile(f) && filesize(f) == parse(Int, size) && file_checksum(f) == parse(UInt64, chk)) ||
                    error("checkpoint in $path is torn: $name is not the file its manifest lists (a run was killed inside save!; the directory mixes two saves)")
            end
        end
        nfile = joinpath(path, CKPT_NORMS)
        if isfile(nfile)
            stored = Serialization.deserialize(nfile)
            e_norms = restore(e_norms, stored.e_norm)
            n_norms = restore(n_norms, stored.n_norm)
            o_norms = restore(o_norms, stored.o_norm)
        else
            online(n) = n isa NormaliserOnline || (n isa AbstractDict && any(online, values(n)))
            (online(e_norms) || online(n_norms) || online(o_norms)) &&
                error("checkpoint in $path has no $CKPT_NORMS: its online normalisers' statistics were not saved and cannot be rebuilt")
        end
        ofile = joinpath(path, CKPT_OPT)
        (opt !== nothing && isfile(ofile)) && (opt_state = Serialization.deserialize(ofile))
        lfile = joinpath(path, CKPT_LOG)
        if isfile(lfile)
            for line in eachline(lfile)
                kind, step, loss = split(line, ',')
                log = kind == "train" ? df_train : df_valid
                push!(log.step, parse(Int, step)); push!(log.loss, parse(Float32, loss))
            end
        end
    end
    mgn = GraphNetwork(quantities, dims, e_norms, n_norms, o_norms, outputs, mps, layer_size, hidden_layers, nothing;
        device = hip_device, ln_mode = ln_mode, ln_dims = ln_dims)
    if have
        ps = Vector{Float32}(undef, param_count(mgn.cfg))
        filesize(pfile) == sizeof(ps) || error("checkpoint $pfile holds $(filesize(pfile)) bytes, this model has $(sizeof(ps))")
        read!(pfile, ps)
    else
        ps = init_params(mgn.cfg)
    end
    mgn.ps = ps
    return mgn, opt_state, df_train, df_valid
end

"""
`save!(mgn, opt_state, df_train, df_valid, step, loss, path; is_training = true)` as called at src/MeshGraphNets.jl:460-471: appends
(step, loss) to the training or the validation log and writes the whole state -- `mgn.ps`, `mgn.e_norm`, `mgn.n_norm`, `mgn.o_norm`
(with whatever an online normaliser has accumulated so far) and `opt_state`.  Every file is written beside its target and renamed, the manifest
(sizes and checksums of the four files) last: a run killed inside `save!` leaves either the previous checkpoint whole or a directory whose
manifest does not match, which `load` refuses instead of mixing the files of two saves.
"""
function save!(mgn::GraphNetwork, opt_state, df_train, df_valid, step, loss, path; is_training = true)
    mkpath(path)
    log = is_training ? df_train : df_valid
    push!(log.step, Int(step)); push!(log.loss, Float32(loss))
    function atomically(f, name)
        tmp = joinpath(path, name * ".tmp")
        f(tmp)
        mv(tmp, joinpath(path, name); force = true)
    end
    atomically(CKPT_NORMS) do tmp
        Serialization.serialize(tmp, (e_norm = snapshot(mgn.e_norm), n_norm = snapshot(mgn.n_norm), o_norm = snapshot(mgn.o_norm)))
    end
    atomically(CKPT_OPT) do tmp
        Serialization.serialize(tmp, opt_state)
    end
    atomically(CKPT_LOG) do tmp
        open(tmp, "w") do io
            for (kind, l) in (("train", df_train), ("valid", df_valid)), i in eachindex(l.step)
                println(io, kind, ',', l.step[i], ',', l.loss[i])
            end
        end
    end
    atomically(CKPT_PARAMS) do tmp
        write(tmp, mgn.ps::Vector{Float32})
    end
    atomically(CKPT_MANIFEST) do tmp            # last: sizes and checksums of the four -- `load` refuses a directory that mixes two saves
        open(tmp, "w") do io
            for name in (CKPT_NORMS, CKPT_OPT, CKPT_LOG, CKPT_PARAMS)
                f = joinpath(path, name)
                println(io, name, ',', filesize(f), ',', file_checksum(f))
            end
        end
    end
    return nothing
end

"sum over the file's bytes b_i (i from 1) of i * b_i, modulo 2^64 (checkpoint.py: file_checksum)"
function file_checksum(fname)
    s = UInt64(0)
    for (i, b) in enumerate(read(fname))
        s += UInt64(i) * UInt64(b)
    end
    return s
end

# ---- graph -----------------------------------------------------------------------------------------------------------------------
"Once per trajectory, where the reference calls create_base_graph (src/MeshGraphNets.jl:360,418,596)."
# Content key of a topology.  The key is taken from the CALLER's arrays (whatever their element type) and by content: an
# `objectid` would name the Int32 copy made below -- a cache that never hits and re-runs mgn_set_graph (receiver sort, CSR,
# buffer reallocation) for every ODE right-hand side -- and, being address based, can match a different array after GC.  The
# reference also mutates `senders` in place while it builds the graph (`senders .+= 1`, src/graph.jl:32): a content hash sees that.
graph_key(senders, receivers, N) = (length(senders), Int(N), hash(senders), hash(receivers))

function set_trajectory_graph!(mgn::GraphNetwork, senders::AbstractVector{<:Integer}, receivers::AbstractVector{<:Integer}, N::Integer;
        mesh_pos::Union{Nothing, Matrix{Float32}} = nothing)
    key = graph_key(senders, receivers, N)
    senders = senders isa Vector{Int32} ? senders : Vector{Int32}(senders)        # convert only when needed
    receivers = receivers isa Vector{Int32} ? receivers : Vector{Int32}(receivers)
    pos = mesh_pos === nothing ? Ptr{Float32}(C_NULL) : pointer(mesh_pos)
    pd = mesh_pos === nothing ? 0 : size(mesh_pos, 1)
    GC.@preserve senders receivers mesh_pos check(mgn.handle,
        ccall((:mgn_set_graph, LIB), Cint,
            (Ptr{Cvoid}, Int32, Int64, Ptr{Int32}, Ptr{Int32}, Int32, Ptr{Float32}, Int32),
            mgn.handle, N, length(senders), senders, receivers, 1 #= Julia indices, src/graph.jl:31-34 =#, pos, pd))
    mgn.graph_key = key
    return mgn
end

sync_graph!(mgn::GraphNetwork, graph, N) =
    graph_key(graph.senders, graph.receivers, N) == mgn.graph_key || set_trajectory_graph!(mgn, graph.senders, graph.receivers, N)

# Called before every forward / step!: the optimiser updates `mgn.ps` in place (src/MeshGraphNets.jl:375-377), so the shim cannot know
# whether it changed.  mgn_set_params compares with what it holds and returns at once when nothing did (0.3 ms for 9 MB); when something
# did it only stores the vector (0.1 ms) -- the kernels' weight layouts are written on the device by the call that needs them.
function sync_params!(mgn::GraphNetwork, packed::Vector{Float32})
    mgn.resident && return                     # (adam_init!: the parameters live on the device; resident_params! brings `ps` up to date)
    check(mgn.handle, ccall((:mgn_set_params, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Csize_t), mgn.handle, packed, length(packed)))
    return
end

# ---- the model: mgn.model(graph, ps, st) at src/solve.jl:200 ----------------------------------------------------------------------
"`ps` is the packed Vector{Float32} (see pack_params)."
function forward(mgn::GraphNetwork, graph::FeatureGraph, ps::Vector{Float32})
    sync_params!(mgn, ps)
    N = size(graph.nf, 2)
    sync_graph!(mgn, graph, N)
    out = Matrix{Float32}(undef, mgn.cfg.O, N)
    nf = Array(graph.nf); ef = Array(graph.ef)             # host arrays: the engine copies in (H2D) itself
    GC.@preserve nf ef out check(mgn.handle,
        ccall((:mgn_forward, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}), mgn.handle, nf, ef, out))
    return out
end

"""
Pullback of the model call: `(out, nfbar, gs) = forward_vjp(mgn, graph, ps, ybar)` with nfbar = ybar' d out / d nf (Fn x N) and
gs = ybar' d out / d ps (packed).  One forward with kept activations + one reverse pass on the device (mgn_forward_vjp).
"""
function forward_vjp(mgn::GraphNetwork, graph::FeatureGraph, ps::Vector{Float32}, ybar::AbstractMatrix)
    sync_params!(mgn, ps)
    N = size(graph.nf, 2)
    sync_graph!(mgn, graph, N)
    out = Matrix{Float32}(undef, mgn.cfg.O, N)
    nfbar = Matrix{Float32}(undef, mgn.cfg.Fn, N)
    gs = Vector{Float32}(undef, length(ps))
    nf = Array(graph.nf); ef = Array(graph.ef); yb = Matrix{Float32}(ybar)
    GC.@preserve nf ef yb out nfbar gs check(mgn.handle,
        ccall((:mgn_forward_vjp, LIB), Cint,
            (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Csize_t),
            mgn.handle, nf, ef, yb, out, nfbar, gs, length(gs)))
    return out, nfbar, gs
end

# What Zygote sees when it differentiates ode_func_train / train_loss as written (src/strategies.jl:175-196): the normalisers,
# build_graph, inverse_data and `.* val_mask` around the model are Julia code and are differentiated by Zygote; the model itself is
# this rule.  The forward pass of the rule is the plain inference path; the reverse pass re-runs the forward with kept activations
# (mgn_forward_vjp) -- the sensitivity algorithm calls the pullback once per right-hand side it unwinds.
# The edge features are constants of a trajectory (create_base_graph, src/graph.jl:25-55): their cotangent is zero.
function ChainRulesCore.rrule(::typeof(forward), mgn::GraphNetwork, graph::FeatureGraph, ps::Vector{Float32})
    out = forward(mgn, graph, ps)
    function forward_pullback(ybar)
        _, nfbar, gs = forward_vjp(mgn, graph, ps, ChainRulesCore.unthunk(ybar))
        gbar = Tangent{typeof(graph)}(; nf = nfbar, ef = ZeroTangent(), senders = NoTangent(), receivers = NoTangent())
        return NoTangent(), NoTangent(), gbar, gs
    end
    return out, forward_pullback
end

# ---- step!: src/strategies.jl:418-422, consumed at src/MeshGraphNets.jl:370-378 ----------------------------------------------------
"""
`step!(mgn, graph, target, mask, loss_function)`: returns `(gs, loss)` with `loss = mean(mse_reduce(target, output)[mask])`.
`gs` is a ONE-ELEMENT TUPLE holding the packed gradient (the order of `pack_params`), so the caller's loop
`for i in eachindex(gs); opt_state, ps = Optimisers.update(opt_state, mgn.ps, gs[i]); mgn.ps = ps; end`
(src/MeshGraphNets.jl:375-377) runs unchanged: one `Optimisers.update` on the packed vector.
`mask` are the Int32 node indices built at src/MeshGraphNets.jl:352 (1-based).  Only `mse_reduce` runs on the device.
`mgn_step` copies with hipMemcpyDefault: with AMDGPU.jl arrays pass `pointer(graph.nf)` etc. of the ROCArrays and a
`ROCVector{Float32}` for `gs` instead of the host copies made below, and the gradients never cross PCIe (the
reference keeps graph, ps and gs on the GPU, src/MeshGraphNets.jl:255-263); `mask` stays a host vector.
On a partitioned mesh (`nranks > 1`, after `comm_init!`; one edge set) every rank calls `step!` with the GLOBAL graph, target and
mask, exactly as above, and every rank gets the complete gradient and the loss of the whole mesh with the same bits -- each rank's
`Optimisers.update` then yields the same parameters and no broadcast is needed.  The library exchanges the halo rows (forward) and
their gradients (reverse) and adds the ranks' gradients in rank order; the same `ccall`, nothing else changes on the Julia side.
"""
function step!(mgn::GraphNetwork, graph::FeatureGraph, target::AbstractMatrix, mask::AbstractVector{<:Integer}, loss_function = nothing)
    ps = mgn.ps::Vector{Float32}
    sync_params!(mgn, ps)
    N = size(graph.nf, 2)
    sync_graph!(mgn, graph, N)
    gs = Vector{Float32}(undef, length(ps))
    loss = Ref{Float32}(0)
    nf = Array(graph.nf); ef = Array(graph.ef); tg = Matrix{Float32}(Array(target)); mk = Vector{Int32}(Array(mask))
    GC.@preserve nf ef tg mk gs check(mgn.handle,
        ccall((:mgn_step, LIB), Cint,
            (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Int32}, Int64, Int32, Ptr{Float32}, Csize_t, Ref{Float32}),
            mgn.handle, nf, ef, tg, mk, length(mk), 1, gs, length(gs), loss))
    return (gs,), loss[]
end

"Per-feature (sum, sum of squares) in Float64 of `x` (dim x rows): one accumulation step of a `NormaliserOnline`, on the device."
function feature_stats(mgn::GraphNetwork, x::Matrix{Float32})
    dim, rows = size(x)
    s = zeros(Float64, dim); q = zeros(Float64, dim)
    GC.@preserve x s q check(mgn.handle,
        ccall((:mgn_feature_stats, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Int64, Int32, Ptr{Float64}, Ptr{Float64}),
            mgn.handle, x, rows, dim, s, q))
    return s, q
end

# ---- derivative training on a device-resident trajectory: src/MeshGraphNets.jl:364-378 over src/strategies.jl:395-416 ---------------
"""
`train_trajectory!(mgn, frames, dt, node_type_onehot, edge_features; noise_stddev, noisy_nodes, seed)`: once per trajectory, after
`set_trajectory_graph!` -- what `add_targets!` and `preprocess!` (src/dataset.jl:461-509) do for the derivative strategies, on the
device.  `frames` is O x N x T: `vcat([data[field] for field in target_fields]...)` of every frame, the last one only ever a target;
`dt` is `meta["dt"]`, a number or the vector of times.  `noise_stddev` (length O) and `noisy_nodes` (length N, nonzero = noisy;
`nothing` = every node) replace the noise `preprocess!` adds to `data[field]`; the targets carry none.
`step_datapoint!(mgn, datapoint, mask; accumulate)` is then `init_train_step` + `step!` for `datapoint` (1-based, as the loop
`for datapoint in 1:delta` counts): it returns `((gs,), loss)` as `step!` does, so `Optimisers.update` runs unchanged on `gs[1]`.
`online_norms!(mgn; node, edge, out, max_acc, std_epsilon)` switches normalisers to `NormaliserOnline` on the device; with
`accumulate = true` a step adds its raw rows to their totals and renews their maps first.  `norm_state` / `norm_state!` read and
restore one group's totals (0 node state columns, 1 edge features, 2 output) for `save!` / `load`; `datapoint_export` returns the
arrays a step consumes.
"""
function train_trajectory!(mgn::GraphNetwork, frames::Array{Float32, 3}, dt, node_type_onehot::Union{Nothing, Matrix{Float32}},
        edge_features::Matrix{Float32}; noise_stddev::Union{Nothing, Vector{Float32}} = nothing,
        noisy_nodes::Union{Nothing, AbstractVector} = nothing, seed::Integer = 0)
    T = size(frames, 3)
    times = dt isa AbstractArray ? Vector{Float32}(vec(dt)) : nothing
    step = times === nothing ? Float32(dt) : 0.0f0
    GC.@preserve frames times node_type_onehot edge_features check(mgn.handle,
        ccall((:mgn_train_set_trajectory, LIB), Cint,
            (Ptr{Cvoid}, Ptr{Float32}, Int32, Ptr{Float32}, Float32, Ptr{Float32}, Ptr{Float32}),
            mgn.handle, frames, T, opt_ptr(times), step, opt_ptr(node_type_onehot), edge_features))
    noisy = noisy_nodes === nothing ? nothing : Vector{UInt8}(noisy_nodes .!= 0)
    nz = noisy === nothing ? Ptr{UInt8}(C_NULL) : pointer(noisy)
    GC.@preserve noise_stddev noisy check(mgn.handle,
        ccall((:mgn_train_set_noise, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{UInt8}, UInt64),
            mgn.handle, opt_ptr(noise_stddev), nz, UInt64(seed)))
    return mgn
end

function step_datapoint!(mgn::GraphNetwork, datapoint::Integer, mask::AbstractVector{<:Integer}; accumulate::Bool = false)
    ps = mgn.ps::Vector{Float32}
    sync_params!(mgn, ps)
    gs = Vector{Float32}(undef, length(ps))
    loss = Ref{Float32}(0)
    mk = Vector{Int32}(Array(mask))
    GC.@preserve mk gs check(mgn.handle,
        ccall((:mgn_step_datapoint, LIB), Cint,
            (Ptr{Cvoid}, Int32, Int32, Ptr{Int32}, Int64, Int32, Ptr{Float32}, Csize_t, Ref{Float32}),
            mgn.handle, datapoint - 1, accumulate ? 1 : 0, mk, length(mk), 1, gs, length(gs), loss))
    return (gs,), loss[]
end

"""
`step!` on the block-diagonal graph of the datapoints `datapoints` (1-based, repeats allowed, at most 64) of the resident trajectory with
the mask repeated per copy (`Args.batchsize`): `((gs,), loss, losses)` with `loss` the mean of the per-datapoint `losses` and `gs`
its gradient.  `accumulate`: the online normalisers take all the datapoints first, then every one is normalised with the result.
"""
function step_datapoints!(mgn::GraphNetwork, datapoints::AbstractVector{<:Integer}, mask::AbstractVector{<:Integer}; accumulate::Bool = false)
    ps = mgn.ps::Vector{Float32}
    sync_params!(mgn, ps)
    gs = Vector{Float32}(undef, length(ps))
    loss = Ref{Float32}(0)
    dp = Vector{Int32}(Array(datapoints) .- 1)
    losses = zeros(Float32, max(length(dp), 1))
    mk = Vector{Int32}(Array(mask))
    GC.@preserve dp mk gs losses check(mgn.handle,
        ccall((:mgn_step_datapoints, LIB), Cint,
            (Ptr{Cvoid}, Ptr{Int32}, Int32, Int32, Ptr{Int32}, Int64, Int32, Ptr{Float32}, Csize_t, Ref{Float32}, Ptr{Float32}),
            mgn.handle, dp, length(dp), accumulate ? 1 : 0, mk, length(mk), 1, gs, length(gs), loss, losses))
    return (gs,), loss[], losses[1:length(dp)]
end

# ---- parameters that stay on the device, and Optimisers.Adam there (opt-in) ---------------------------------------------------------
mutable struct MgnAdamDesc   # mirrors `mgn_adam_desc` (include/mgn_hip.h), field for field
    eta::Float32
    beta1::Float32
    beta2::Float32
    epsilon::Float32
end

"New parameters from `packed`, a host `Vector{Float32}` or a device array's pointer (no host work, no synchronisation for the latter)."
function set_params_dev!(mgn::GraphNetwork, packed::Union{Vector{Float32}, Ptr{Float32}}, n::Integer = length(mgn.ps))
    GC.@preserve packed check(mgn.handle,
        ccall((:mgn_set_params_dev, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Csize_t), mgn.handle, packed, n))
    return mgn
end

"The parameters as they stand on the device into `packed` (a host vector or a device array's pointer)."
function get_params_dev!(mgn::GraphNetwork, packed::Union{Vector{Float32}, Ptr{Float32}}, n::Integer = length(mgn.ps))
    GC.@preserve packed check(mgn.handle,
        ccall((:mgn_get_params_dev, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Csize_t), mgn.handle, packed, n))
    return packed
end

"`mgn.ps` brought up to date with the device (before `save!`, or to leave the resident mode by hand)."
resident_params!(mgn::GraphNetwork) = (get_params_dev!(mgn, mgn.ps::Vector{Float32}); mgn.ps)

"""
`Optimisers.setup(Optimisers.Adam(eta, beta, epsilon), mgn.ps)` on the device, opt-in: the parameters `mgn.ps` go to the engine once and
live there from now on (`mgn.ps` is no longer handed over before a call; `resident_params!` reads them back), so that the loop of
src/MeshGraphNets.jl:364-378 becomes `gs, loss = step_datapoint!(mgn, t, mask); adam_update!(mgn, gs)`: no parameters cross PCIe and
no layouts are described on the host per iteration (the gradient still does while `step_datapoint!` returns a host vector; a caller
that holds a device array hands `adam_update!` its pointer).
"""
function adam_init!(mgn::GraphNetwork; eta::Real = 1.0f-3, beta = (0.9f0, 0.999f0), epsilon::Real = 1.0f-8)
    set_params_dev!(mgn, mgn.ps::Vector{Float32})
    mgn.resident = true
    d = MgnAdamDesc(Float32(eta), Float32(beta[1]), Float32(beta[2]), Float32(epsilon))
    # (@ccall: tests/test_params_dev_host.py looks for this call)
    rc = @ccall LIB.mgn_adam_init(mgn.handle::Ptr{Cvoid}, d::Ref{MgnAdamDesc})::Cint
    check(mgn.handle, rc)
    return mgn
end

"`Optimisers.update` on the device: `gs` is what `step!` / `step_datapoint!` returned (`(gs,)` or the vector), or a device array's pointer."
function adam_update!(mgn::GraphNetwork, gs)
    g = gs isa Tuple ? gs[1] : gs
    GC.@preserve g check(mgn.handle,
        ccall((:mgn_adam_update, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Csize_t), mgn.handle, g, length(mgn.ps)))
    return mgn
end

"(mt, vt, beta_t) of the device Adam: Float32 moments and the Float64 powers of beta, as `Optimisers` keeps them per leaf."
function adam_state(mgn::GraphNetwork)
    n = length(mgn.ps)
    mt = Vector{Float32}(undef, n); vt = Vector{Float32}(undef, n); bt = zeros(Float64, 2)
    GC.@preserve mt vt bt check(mgn.handle,
        ccall((:mgn_adam_state, LIB), Cint, (Ptr{Cvoid}, Int32, Ptr{Float32}, Ptr{Float32}, Ptr{Float64}), mgn.handle, 0, mt, vt, bt))
    return mt, vt, bt
end

function adam_state!(mgn::GraphNetwork, mt::Vector{Float32}, vt::Vector{Float32}, beta_t::Vector{Float64})
    GC.@preserve mt vt beta_t check(mgn.handle,
        ccall((:mgn_adam_state, LIB), Cint, (Ptr{Cvoid}, Int32, Ptr{Float32}, Ptr{Float32}, Ptr{Float64}), mgn.handle, 1, mt, vt, beta_t))
    return mgn
end

function online_norms!(mgn::GraphNetwork; node::Bool = true, edge::Bool = true, out::Bool = true, max_acc::Real = 1e6,
        std_epsilon::Real = 1.0f-8)
    check(mgn.handle, ccall((:mgn_train_online_norms, LIB), Cint, (Ptr{Cvoid}, Int32, Int32, Int32, Float64, Float32),
        mgn.handle, node ? 1 : 0, edge ? 1 : 0, out ? 1 : 0, Float64(max_acc), Float32(std_epsilon)))
    return mgn
end

norm_dim(mgn::GraphNetwork, group::Integer) = group == 1 ? Int(mgn.cfg.Fe) : Int(mgn.cfg.O)

"(sum, sum_squares, count, calls) of an online group, Float64 as on the device."
function norm_state(mgn::GraphNetwork, group::Integer)
    s = zeros(Float64, norm_dim(mgn, group)); q = zeros(Float64, norm_dim(mgn, group)); cc = zeros(Float64, 2)
    GC.@preserve s q cc check(mgn.handle,
        ccall((:mgn_train_norm_state, LIB), Cint, (Ptr{Cvoid}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
            mgn.handle, group, 0, s, q, cc))
    return s, q, cc[1], cc[2]
end

function norm_state!(mgn::GraphNetwork, group::Integer, s::Vector{Float64}, q::Vector{Float64}, count::Real, calls::Real)
    cc = Float64[count, calls]
    GC.@preserve s q cc check(mgn.handle,
        ccall((:mgn_train_norm_state, LIB), Cint, (Ptr{Cvoid}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
            mgn.handle, group, 1, s, q, cc))
    return mgn
end

"(nf Fn x N, ef Fe x E, target O x N) of `datapoint` (1-based): normalised as the step consumes them, or raw."
function datapoint_export(mgn::GraphNetwork, datapoint::Integer, N::Integer, E::Integer; normalised::Bool = true)
    nf = Matrix{Float32}(undef, mgn.cfg.Fn, N); ef = Matrix{Float32}(undef, mgn.cfg.Fe, E); tg = Matrix{Float32}(undef, mgn.cfg.O, N)
    GC.@preserve nf ef tg check(mgn.handle,
        ccall((:mgn_datapoint_export, LIB), Cint, (Ptr{Cvoid}, Int32, Int32, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}),
            mgn.handle, datapoint - 1, normalised ? 1 : 0, nf, ef, tg))
    return nf, ef, tg
end

# ---- fused right-hand side and native rollout (optional fast paths) ---------------------------------------------------------------
opt_ptr(x::Nothing) = Ptr{Float32}(C_NULL)
opt_ptr(x::Array{Float32}) = pointer(x)

"""
Frozen normalisers as per-feature affine maps (mgn_set_norms): forward `y = x * scale + shift` for node and edge features,
`inverse_data(o_norm, y) = y * out_scale + out_shift` for the outputs.  `nothing` = identity.  Needed by ode_step_fused,
ode_step_resident, native_rollout and ode_vjp -- not by `mgn.model` / `step!`, whose FeatureGraph arrives normalised.
"""
function set_norms!(mgn::GraphNetwork; node_scale = nothing, node_shift = nothing, edge_scale = nothing, edge_shift = nothing,
        out_scale = nothing, out_shift = nothing)
    GC.@preserve node_scale node_shift edge_scale edge_shift out_scale out_shift check(mgn.handle,
        ccall((:mgn_set_norms, LIB), Cint,
            (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}),
            mgn.handle, opt_ptr(node_scale), opt_ptr(node_shift), opt_ptr(edge_scale), opt_ptr(edge_shift), opt_ptr(out_scale), opt_ptr(out_shift)))
    return mgn
end

"""
`freeze_norms!(mgn, fields, target_fields, dims)`: derive the affine maps from the normaliser OBJECTS the reference built
(src/MeshGraphNets.jl:79-203) by evaluating each on a column of zeros and a column of ones -- every GraphNetCore normaliser is
affine once frozen, so scale = n(1) - n(0), shift = n(0), whatever its fields are called -- and install them (set_norms!).
Call it after the online normalisers have stopped accumulating (`norm_steps` passed; evaluation runs: always), since calling an
accumulating NormaliserOnline feeds it the probe.  `fields`: node fields in build_graph's order (src/graph.jl:80-86; `node_type`
is appended last there and here); `dims[f]`: rows of field f.
"""
function freeze_norms!(mgn::GraphNetwork, fields, target_fields, dims::AbstractDict)
    probe(n, d) = (z = vec(Float32.(Array(n(zeros(Float32, d, 1))))); o = vec(Float32.(Array(n(ones(Float32, d, 1))))); (o .- z, z))
    ns, nsh = Float32[], Float32[]
    for f in vcat(fields, "node_type")
        s, sh = probe(mgn.n_norm[f], dims[f]); append!(ns, s); append!(nsh, sh)
    end
    es, esh = probe(mgn.e_norm, Int(mgn.cfg.Fe))
    os, osh = Float32[], Float32[]
    for f in target_fields      # inverse_data(o_norm, y) = y * scale + shift, probed the same way
        inv(y) = inverse_data(mgn.o_norm[f], y)
        s, sh = probe(inv, dims[f]); append!(os, s); append!(osh, sh)
    end
    return set_norms!(mgn; node_scale = ns, node_shift = nsh, edge_scale = es, edge_shift = esh, out_scale = os, out_shift = osh)
end

"""
Once per trajectory (where `create_base_graph` returns, src/MeshGraphNets.jl:360,418,596): make the static RHS
inputs device-resident and run the edge encoder once.  Afterwards `ode_step_resident(mgn, x)` moves only the state.
"""
function set_static!(mgn::GraphNetwork, node_type_onehot::Matrix{Float32}, edge_features::Matrix{Float32},
        val_mask_row::Union{Nothing, Vector{Float32}} = nothing)
    GC.@preserve node_type_onehot edge_features val_mask_row check(mgn.handle,
        ccall((:mgn_set_static, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}),
            mgn.handle, node_type_onehot, edge_features, opt_ptr(val_mask_row)))
    return mgn
end

function ode_step_resident(mgn::GraphNetwork, x::Matrix{Float32})
    out = similar(x)
    GC.@preserve x out check(mgn.handle,
        ccall((:mgn_ode_step, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}),
            mgn.handle, x, C_NULL, C_NULL, C_NULL, out))
    return out
end

"""
Fused right-hand side: everything `ode_step` does after the state split (src/solve.jl:198-218) in one call --
build_graph normalisation, model, inverse_data, `.* val_mask`.  Normalisers must have been frozen into affine
maps (set_norms! / freeze_norms!).
"""
function ode_step_fused(mgn::GraphNetwork, x::Matrix{Float32}, node_type_onehot::Matrix{Float32},
        edge_features::Matrix{Float32}, val_mask_row::Vector{Float32})
    out = similar(x)
    GC.@preserve x node_type_onehot edge_features val_mask_row out check(mgn.handle,
        ccall((:mgn_ode_step, LIB), Cint,
            (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}),
            mgn.handle, x, node_type_onehot, edge_features, val_mask_row, out))
    return out
end

"""
`lambda' df/dx` and `lambda' df/dps` of the fused right-hand side f = ode_step_fused (mgn_ode_vjp): the hand-written form of what
the rrule above gives Zygote piecewise, for callers that write their own adjoint of `solve`.  Returns (xbar, gs, f(x)).
"""
function ode_vjp(mgn::GraphNetwork, x::Matrix{Float32}, node_type_onehot::Matrix{Float32}, edge_features::Matrix{Float32},
        val_mask_row::Union{Nothing, Vector{Float32}}, lambda::Matrix{Float32})
    ps = mgn.ps::Vector{Float32}
    sync_params!(mgn, ps)
    dxdt = similar(x); xbar = similar(x); gs = Vector{Float32}(undef, length(ps))
    GC.@preserve x node_type_onehot edge_features val_mask_row lambda dxdt xbar gs check(mgn.handle,
        ccall((:mgn_ode_vjp, LIB), Cint,
            (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Csize_t),
            mgn.handle, x, node_type_onehot, edge_features, opt_ptr(val_mask_row), lambda, dxdt, xbar, gs, length(gs)))
    return xbar, gs, dxdt
end

# ---- explicit Runge-Kutta by tableau (mgn_erk_named, the *_erk entry points): the reference types every solver argument as
# OrdinaryDiffEqAlgorithm, so RK4(), BS3(), DP5(), Heun(), Midpoint() or Ralston() may arrive where Euler() and Tsit5() do
const ERK_NAMES = (Euler = 0, Heun = 1, Midpoint = 2, Ralston = 3, RK4 = 4, BS3 = 5, DP5 = 6, Tsit5 = 7)
const ERK_EMBEDDED = (:BS3, :DP5, :Tsit5)
const ERK_TABLEAU_DOUBLES = 76

"the flat tableau (include/mgn_hip.h, MGN_ERK_TABLEAU_DOUBLES) of a named method"
function erk_named(name::Symbol)
    haskey(ERK_NAMES, name) || throw(ArgumentError("no tableau named $name; the names are $(keys(ERK_NAMES))"))
    tab = zeros(Float64, ERK_TABLEAU_DOUBLES)
    rc = ccall((:mgn_erk_named, LIB), Cint, (Int32, Ptr{Float64}), Int32(ERK_NAMES[name]), tab)
    rc == 0 || throw(ArgumentError("mgn_erk_named($name) returned $rc"))
    ccall((:mgn_erk_check, LIB), Cint, (Ptr{Float64},), tab) == 0 || throw(ArgumentError("the tableau of $name does not pass mgn_erk_check"))
    return tab
end

# the tableau a rollout of `name` goes through (nothing: Euler and Tsit5 keep mgn_rollout's own solvers), and its step mode: a method
# with an embedded pair follows Tsit5's rule (adaptive unless fixed_step with a dt given), one without steps by dt
erk_route(name::Symbol) = name in (:Euler, :Tsit5) ? nothing : erk_named(name)
erk_adaptive(name::Symbol, dt, fixed_step) = Int32(name in ERK_EMBEDDED && !(fixed_step && dt !== nothing) ? 1 : 0)

"""
    native_rollout(solver, mgn, x0, node_type_onehot, edge_features, val_mask_row, inflow_mask_row, inflow_data, start, stop, dt, saves)
        -> (sol_u::Vector{Matrix{Float32}}, sol_t)

`rollout` of src/solve.jl:42-68 on the device (mgn_rollout): the ODEProblem over `ode_func_eval` solved with fixed-step Euler
(`dt` given: `solve(prob, solver; adaptive = false, dt = dt, saveat = saves)`) or adaptive Tsit5 (`dt === nothing`:
`solve(prob, solver; saveat = saves, tstops = saves)`), no host round trip per right-hand side.  `solver` is `:Euler`, `:Tsit5` or
an OrdinaryDiffEq algorithm object of those names.  The reference's own branch (src/solve.jl:57-61) is on `dt` alone, whatever the
solver: `fixed_step = true` is that branch for `:Tsit5` with a `dt` given (`adaptive = false, dt = dt`: fixed steps that need not divide
the save spacing, saves from the dense output; MGN_SOLVER_TSIT5_FIXED); the default `false` keeps the results this function has always
returned (adaptive Tsit5 with `dt` as its first step).  `:Euler` ignores it.  The inflow frame of a right-hand side is the reference's own
`floor(Int, t / saves_dt) + 1` in the element type of `saves` (src/solve.jl:151; MGN_INFLOW_REFERENCE), `inflow_data` being
(O x N x frames).  Needs frozen normalisers (freeze_norms!) and the trajectory's graph (set_trajectory_graph!).
`:Heun`, `:Midpoint`, `:Ralston`, `:RK4`, `:BS3`, `:DP5` (or the OrdinaryDiffEq objects of those names) go through mgn_rollout_erk with
mgn_erk_named's tableau: `:BS3` and `:DP5` follow Tsit5's rule (adaptive unless `fixed_step` with a `dt`), the others step by `dt`;
fixed steps of a tableau need `saves_dt / dt` integral.
"""
function native_rollout(solver, mgn::GraphNetwork, x0::Matrix{Float32}, node_type_onehot::Matrix{Float32}, edge_features::Matrix{Float32},
        val_mask_row::Union{Nothing, Vector{Float32}}, inflow_mask_row::Union{Nothing, Vector{UInt8}},
        inflow_data::Union{Nothing, Array{Float32, 3}}, start, stop, dt, saves; abstol = 1.0f-6, reltol = 1.0f-3, tolerant_inflow = false,
        fixed_step = false)
    name = solver isa Symbol ? solver : nameof(typeof(solver))
    haskey(ERK_NAMES, name) || throw(ArgumentError("native_rollout drives Euler, Tsit5, Heun, Midpoint, Ralston, RK4, BS3 and DP5; got $name"))
    erk = erk_route(name)
    sync_params!(mgn, mgn.ps::Vector{Float32})
    O, N = size(x0)
    ns = length(saves)
    out = Array{Float32, 3}(undef, O, N, ns)
    sdt = ns > 1 ? saves[2] - saves[1] : one(eltype(saves))
    f64 = eltype(saves) == Float64
    d = MgnRolloutDesc(name == :Euler ? 0 : (fixed_step ? 2 : 1), start, stop, dt === nothing ? 0 : dt, sdt, ns, abstol, reltol,
        pointer(x0), pointer(node_type_onehot), pointer(edge_features), opt_ptr(val_mask_row),
        inflow_mask_row === nothing ? Ptr{UInt8}(C_NULL) : pointer(inflow_mask_row), inflow_data === nothing ? Ptr{Float32}(C_NULL) : pointer(inflow_data),
        inflow_data === nothing ? 0 : size(inflow_data, 3), pointer(out), 0, 0, 0, tolerant_inflow ? 1 : 0, f64 ? 1 : 0,
        start, stop, dt === nothing ? 0 : dt, sdt)
    if erk === nothing
        GC.@preserve x0 node_type_onehot edge_features val_mask_row inflow_mask_row inflow_data out check(mgn.handle,
            ccall((:mgn_rollout, LIB), Cint, (Ptr{Cvoid}, Ref{MgnRolloutDesc}), mgn.handle, d))
    else      # (d.solver is not read)
        GC.@preserve x0 node_type_onehot edge_features val_mask_row inflow_mask_row inflow_data out erk check(mgn.handle,
            ccall((:mgn_rollout_erk, LIB), Cint, (Ptr{Cvoid}, Ref{MgnRolloutDesc}, Ptr{Float64}, Int32), mgn.handle, d, erk,
                erk_adaptive(name, dt, fixed_step)))
    end
    return [out[:, :, i] for i in 1:ns], collect(saves)
end

"""
    solver_grad(mgn, x0, node_type_onehot, edge_features, val_mask_row, inflow_mask_row, inflow_data, gt, start, stop, dt, saves;
                loss_scale = nothing, cont_target = nothing, cont_weight = 0f0) -> (gs, loss, pred::Array{Float32, 3})

Loss and gradient of ONE fixed-step Euler solve of `ode_func_train` (src/solve.jl:101-117) on the device (mgn_solver_grad): the time
grid, inflow frames and save rule of `native_rollout` with `dt` given, the inflow rows written into a copy the right-hand side sees,
`loss = mean(((gt - pred) .* loss_scale) .^ 2 .* val_mask) + cont_weight * sum(abs, pred[:, :, end] - cont_target)`, gt (O x N x saves).
`gs` is the discrete adjoint -- the exact gradient of that loss of the computed Euler solution, what ReverseDiffAdjoint / ZygoteAdjoint
give -- not InterpolatingAdjoint's continuous approximation.  One upload of the statics, no host work per step, one synchronisation.
"""
function solver_grad(mgn::GraphNetwork, x0::Matrix{Float32}, node_type_onehot::Matrix{Float32}, edge_features::Matrix{Float32},
        val_mask_row::Union{Nothing, Vector{Float32}}, inflow_mask_row::Union{Nothing, Vector{UInt8}},
        inflow_data::Union{Nothing, Array{Float32, 3}}, gt::Array{Float32, 3}, start, stop, dt, saves;
        loss_scale::Union{Nothing, Vector{Float32}} = nothing, cont_target::Union{Nothing, Matrix{Float32}} = nothing, cont_weight = 0.0f0,
        tolerant_inflow = false)
    ps = mgn.ps::Vector{Float32}
    sync_params!(mgn, ps)
    O, N = size(x0)
    ns = length(saves)
    size(gt, 3) >= ns || throw(DimensionMismatch("gt has $(size(gt, 3)) frames, the solve saves $ns"))
    g = Array{Float32, 3}(gt[:, :, 1:ns])
    out = Array{Float32, 3}(undef, O, N, ns)
    gs = Vector{Float32}(undef, length(ps))
    loss = Ref{Float32}(0)
    sdt = ns > 1 ? saves[2] - saves[1] : one(eltype(saves))
    f64 = eltype(saves) == Float64
    d = MgnRolloutDesc(0, start, stop, dt, sdt, ns, 0, 0,
        pointer(x0), pointer(node_type_onehot), pointer(edge_features), opt_ptr(val_mask_row),
        inflow_mask_row === nothing ? Ptr{UInt8}(C_NULL) : pointer(inflow_mask_row), inflow_data === nothing ? Ptr{Float32}(C_NULL) : pointer(inflow_data),
        inflow_data === nothing ? 0 : size(inflow_data, 3), pointer(out), 0, 0, 0, tolerant_inflow ? 1 : 0, f64 ? 1 : 0,
        start, stop, dt, sdt)
    GC.@preserve x0 node_type_onehot edge_features val_mask_row inflow_mask_row inflow_data out g loss_scale cont_target gs check(mgn.handle,
        ccall((:mgn_solver_grad, LIB), Cint,
            (Ptr{Cvoid}, Ref{MgnRolloutDesc}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Float32, Ptr{Float32}, Csize_t, Ref{Float32}),
            mgn.handle, d, g, opt_ptr(loss_scale), opt_ptr(cont_target), Float32(cont_weight), gs, length(gs), loss))
    return gs, loss[], out
end

"""
    solver_grad_tsit5(mgn, x0, node_type_onehot, edge_features, val_mask_row, inflow_mask_row, inflow_data, gt, start, stop, saves;
                      dt = 0, adaptive = true, dense_saves = false, abstol = 1f-6, reltol = 1f-3, loss_scale = nothing,
                      cont_target = nothing, cont_weight = 0f0)
                      -> (gs, loss, pred::Array{Float32, 3}, step_t::Vector{Float64}, step_h::Vector{Float64})

`solver_grad` for Tsit5 (mgn_solver_grad_tsit5): `adaptive = true` is `solve(prob, Tsit5(); saveat = saves, tstops = saves)` with
native_rollout's controller (first step `dt`, 0: Hairer-Wanner); `adaptive = false` is fixed steps of `dt` on solver_grad's time grid.
`dense_saves = true` (MGN_TSIT5_DENSE_SAVES) drops the tstops: `solve(prob, Tsit5(); saveat = saves)`, what the reference's
MultipleShooting calls (src/strategies.jl:343-355) -- the only stop is `stop`, a save no step ends on comes from Tsit5's dense output, and
the adjoint carries its loss term with the steps and interpolation points held fixed; fixed steps then need not divide the save period.
`gs` is the discrete adjoint of the computed solution with the accepted step sequence (returned) held fixed -- not
InterpolatingAdjoint's continuous adjoint.
"""
function solver_grad_tsit5(mgn::GraphNetwork, x0::Matrix{Float32}, node_type_onehot::Matrix{Float32}, edge_features::Matrix{Float32},
        val_mask_row::Union{Nothing, Vector{Float32}}, inflow_mask_row::Union{Nothing, Vector{UInt8}},
        inflow_data::Union{Nothing, Array{Float32, 3}}, gt::Array{Float32, 3}, start, stop, saves;
        dt = zero(eltype(saves)), adaptive = true, dense_saves = false, abstol = 1.0f-6, reltol = 1.0f-3,
        loss_scale::Union{Nothing, Vector{Float32}} = nothing, cont_target::Union{Nothing, Matrix{Float32}} = nothing, cont_weight = 0.0f0,
        tolerant_inflow = false)
    ps = mgn.ps::Vector{Float32}
    sync_params!(mgn, ps)
    O, N = size(x0)
    ns = length(saves)
    size(gt, 3) >= ns || throw(DimensionMismatch("gt has $(size(gt, 3)) frames, the solve saves $ns"))
    g = Array{Float32, 3}(gt[:, :, 1:ns])
    out = Array{Float32, 3}(undef, O, N, ns)
    gs = Vector{Float32}(undef, length(ps))
    loss = Ref{Float32}(0)
    sdt = ns > 1 ? saves[2] - saves[1] : one(eltype(saves))
    f64 = eltype(saves) == Float64
    cap = adaptive ? 4096 : round(Int, (stop - start) / dt) + 2
    while true
        st = Vector{Float64}(undef, cap); sh = Vector{Float64}(undef, cap)
        d = MgnRolloutDesc(1, start, stop, dt, sdt, ns, abstol, reltol,
            pointer(x0), pointer(node_type_onehot), pointer(edge_features), opt_ptr(val_mask_row),
            inflow_mask_row === nothing ? Ptr{UInt8}(C_NULL) : pointer(inflow_mask_row), inflow_data === nothing ? Ptr{Float32}(C_NULL) : pointer(inflow_data),
            inflow_data === nothing ? 0 : size(inflow_data, 3), pointer(out), 0, 0, 0, tolerant_inflow ? 1 : 0, f64 ? 1 : 0,
            start, stop, dt, sdt)
        o = MgnSolverGradOpts((adaptive ? 1 : 0) | (dense_saves ? 2 : 0), cap, pointer(st), pointer(sh), 0, 0, 0)
        # (@ccall: tests/test_solver_train_tsit5_host.py checks this call against the header)
        rc = GC.@preserve x0 node_type_onehot edge_features val_mask_row inflow_mask_row inflow_data out g loss_scale cont_target gs st sh @ccall LIB.mgn_solver_grad_tsit5(
            mgn.handle::Ptr{Cvoid}, d::Ref{MgnRolloutDesc}, o::Ref{MgnSolverGradOpts}, g::Ptr{Float32}, opt_ptr(loss_scale)::Ptr{Float32},
            opt_ptr(cont_target)::Ptr{Float32}, Float32(cont_weight)::Float32, gs::Ptr{Float32}, length(gs)::Csize_t, loss::Ref{Float32})::Cint
        check(mgn.handle, rc)
        if o.n_steps <= cap
            return gs, loss[], out, st[1:o.n_steps], sh[1:o.n_steps]
        end
        cap = o.n_steps          # the record was cut: again with room for every step (the call is bitwise repeatable)
    end
end

"""
    solver_grad_erk(name, mgn, x0, node_type_onehot, edge_features, val_mask_row, inflow_mask_row, inflow_data, gt, start, stop, dt, saves;
                    loss_scale = nothing, cont_target = nothing, cont_weight = 0f0) -> (gs, loss, pred, step_t, step_h)

`solver_grad_tsit5(...; adaptive = false)` for the explicit Runge-Kutta method `name` (`:Heun`, `:Midpoint`, `:Ralston`, `:RK4`, `:BS3`,
`:DP5`; also `:Euler`, `:Tsit5`) through mgn_solver_grad_erk and mgn_erk_named's tableau: fixed steps of `dt` (the save spacing must be
a whole number of them), the inflow rows written into copies, `gs` the exact discrete adjoint of the computed solution.
"""
function solver_grad_erk(name::Symbol, mgn::GraphNetwork, x0::Matrix{Float32}, node_type_onehot::Matrix{Float32}, edge_features::Matrix{Float32},
        val_mask_row::Union{Nothing, Vector{Float32}}, inflow_mask_row::Union{Nothing, Vector{UInt8}},
        inflow_data::Union{Nothing, Array{Float32, 3}}, gt::Array{Float32, 3}, start, stop, dt, saves;
        loss_scale::Union{Nothing, Vector{Float32}} = nothing, cont_target::Union{Nothing, Matrix{Float32}} = nothing, cont_weight = 0.0f0,
        tolerant_inflow = false)
    erk = erk_named(name)
    ps = mgn.ps::Vector{Float32}
    sync_params!(mgn, ps)
    O, N = size(x0)
    ns = length(saves)
    size(gt, 3) >= ns || throw(DimensionMismatch("gt has $(size(gt, 3)) frames, the solve saves $ns"))
    g = Array{Float32, 3}(gt[:, :, 1:ns])
    out = Array{Float32, 3}(undef, O, N, ns)
    gs = Vector{Float32}(undef, length(ps))
    loss = Ref{Float32}(0)
    sdt = ns > 1 ? saves[2] - saves[1] : one(eltype(saves))
    f64 = eltype(saves) == Float64
    cap = round(Int, (stop - start) / dt) + 2
    st = Vector{Float64}(undef, cap); sh = Vector{Float64}(undef, cap)
    d = MgnRolloutDesc(0, start, stop, dt, sdt, ns, 0, 0,      # (solver and tolerances are not read)
        pointer(x0), pointer(node_type_onehot), pointer(edge_features), opt_ptr(val_mask_row),
        inflow_mask_row === nothing ? Ptr{UInt8}(C_NULL) : pointer(inflow_mask_row), inflow_data === nothing ? Ptr{Float32}(C_NULL) : pointer(inflow_data),
        inflow_data === nothing ? 0 : size(inflow_data, 3), pointer(out), 0, 0, 0, tolerant_inflow ? 1 : 0, f64 ? 1 : 0,
        start, stop, dt, sdt)
    o = MgnSolverGradOpts(0, cap, pointer(st), pointer(sh), 0, 0, 0)
    rc = GC.@preserve x0 node_type_onehot edge_features val_mask_row inflow_mask_row inflow_data out g loss_scale cont_target gs st sh erk @ccall LIB.mgn_solver_grad_erk(
        mgn.handle::Ptr{Cvoid}, d::Ref{MgnRolloutDesc}, erk::Ptr{Float64}, o::Ref{MgnSolverGradOpts}, g::Ptr{Float32}, opt_ptr(loss_scale)::Ptr{Float32},
        opt_ptr(cont_target)::Ptr{Float32}, Float32(cont_weight)::Float32, gs::Ptr{Float32}, length(gs)::Csize_t, loss::Ref{Float32})::Cint
    check(mgn.handle, rc)
    n = min(o.n_steps, cap)
    return gs, loss[], out, st[1:n], sh[1:n]
end

"""
    shooting_grad(mgn, node_type_onehot, edge_features, val_mask_row, inflow_mask_row, inflow_data, gt, ranges, tsteps, dt;
                  solver = :Euler, cont_weight = 0f0, max_windows_per_pass = 0) -> (gs, loss, pred::Array{Float32, 3})

The summed loss and gradient of the MultipleShooting windows `ranges` (1-based ranges into `gt` and `tsteps`) in one call
(mgn_shooting_grad): window i is `solver_grad` (`solver = :Euler`) or `solver_grad_tsit5(...; adaptive = false)` (`:Tsit5`) from
`gt[:, :, first(rg)]` over `tsteps[rg]`, with the continuity term against `gt[:, :, first(ranges[i + 1])]` for every window but the
last.  Windows with the same step plan run as one batch of graph copies.  `pred` holds every window's saves, in window order.
"""
function shooting_grad(mgn::GraphNetwork, node_type_onehot::Matrix{Float32}, edge_features::Matrix{Float32},
        val_mask_row::Union{Nothing, Vector{Float32}}, inflow_mask_row::Union{Nothing, Vector{UInt8}},
        inflow_data::Union{Nothing, Array{Float32, 3}}, gt::Array{Float32, 3}, ranges, tsteps, dt;
        solver = :Euler, cont_weight = 0.0f0, max_windows_per_pass = 0, tolerant_inflow = false)
    ps = mgn.ps::Vector{Float32}
    sync_params!(mgn, ps)
    O, N, n_gt = size(gt)
    first_ = Int32[first(rg) - 1 for rg in ranges]; last_ = Int32[last(rg) - 1 for rg in ranges]
    t0 = Float64[tsteps[first(rg)] for rg in ranges]; t1 = Float64[tsteps[last(rg)] for rg in ranges]
    out = Array{Float32, 3}(undef, O, N, sum(length, ranges))
    gs = Vector{Float32}(undef, length(ps))
    loss = Ref{Float32}(0)
    sdt = tsteps[2] - tsteps[1]
    f64 = eltype(tsteps) == Float64
    d = MgnRolloutDesc(solver == :Euler ? 0 : 1, 0, 0, dt, sdt, 0, 0, 0,
        Ptr{Float32}(C_NULL), pointer(node_type_onehot), pointer(edge_features), opt_ptr(val_mask_row),
        inflow_mask_row === nothing ? Ptr{UInt8}(C_NULL) : pointer(inflow_mask_row), inflow_data === nothing ? Ptr{Float32}(C_NULL) : pointer(inflow_data),
        inflow_data === nothing ? 0 : size(inflow_data, 3), pointer(out), 0, 0, 0, tolerant_inflow ? 1 : 0, f64 ? 1 : 0,
        0, 0, dt, sdt)
    s = MgnShootingDesc(length(ranges), pointer(first_), pointer(last_), pointer(t0), pointer(t1), n_gt, 0, max_windows_per_pass, 0, 0, 0)
    # (@ccall: tests/test_shooting_batched_host.py checks this call against the header)
    rc = GC.@preserve node_type_onehot edge_features val_mask_row inflow_mask_row inflow_data out gt gs first_ last_ t0 t1 @ccall LIB.mgn_shooting_grad(
        mgn.handle::Ptr{Cvoid}, d::Ref{MgnRolloutDesc}, s::Ref{MgnShootingDesc}, gt::Ptr{Float32}, C_NULL::Ptr{Float32},
        Float32(cont_weight)::Float32, gs::Ptr{Float32}, length(gs)::Csize_t, loss::Ref{Float32})::Cint
    check(mgn.handle, rc)
    return gs, loss[], out
end

"""
    native_solver_train_step(strategy, mgn, gt, node_type_onehot, edge_features, val_mask_row, inflow_mask_row;
                             n_scale = nothing, inflow_data = gt) -> (gs, loss)

`train_step(::SolverTraining)` / `train_step(::MultipleShooting)` (src/strategies.jl:175-196, 257-292, 312-383) for a strategy with
`Euler()` or `Tsit5()` as its solver, through `solver_grad` / `solver_grad_tsit5` (Tsit5: adaptive unless `solargs.adaptive == false`,
`abstol` / `reltol` from `solargs`, default 1e-6 / 1e-3; every window steps onto its saves unless `dense_saves = true`, which solves
the windows as the reference does -- saveat without tstops, the saves interpolated -- and is not batched): SolverTraining is one solve from `gt[:, :, 1]` over `tstart:dt:tstop` with the field
normaliser's scale `n_scale` in the loss; MultipleShooting one solve per window of the reference's own
`[i:min(T, i + interval_size - 1) for i in 1:(interval_size - 1):(T - 1)]` from `gt[:, :, first(rg)]`, no normaliser, and the continuity
term of window i attached to window i - 1.  The Euler step is `solargs.dt` when given, else `strategy.dt` (the example's
`tstops = tstart:dt:tstop`).  It returns the DISCRETE adjoint (exact gradient of the computed Euler solution), not
InterpolatingAdjoint's continuous approximation the reference defaults to.  Opt-in for `train_network`:
`gs, loss = native_solver_train_step(strategy, mgn, gt, ...)` in place of `train_step(strategy, t)`.  `batched = true` routes a
MultipleShooting strategy with Euler or fixed-step Tsit5 through `shooting_grad` (all windows in one call; the same sum); adaptive
Tsit5 keeps the per-window loop.  A strategy whose solver is `Heun()`, `Midpoint()`, `Ralston()`, `RK4()`, `BS3()` or `DP5()` is served
by `solver_grad_erk` window by window, with fixed steps (`BS3()` and `DP5()` need `adaptive = false` in the solargs).
(Julia is not available where this shim is tested: its ccalls are checked against the header by tests/test_julia_shim.py.)
"""
function native_solver_train_step(strategy, mgn::GraphNetwork, gt::Array{Float32, 3}, node_type_onehot::Matrix{Float32},
        edge_features::Matrix{Float32}, val_mask_row::Union{Nothing, Vector{Float32}}, inflow_mask_row::Union{Nothing, Vector{UInt8}};
        n_scale::Union{Nothing, Vector{Float32}} = nothing, inflow_data::Union{Nothing, Array{Float32, 3}} = gt, batched = false,
        dense_saves = false)
    sname = nameof(typeof(strategy.solver))
    dense_saves && sname != :Tsit5 && throw(ArgumentError("dense_saves is Tsit5's dense output"))
    dense_saves && batched && throw(ArgumentError("dense_saves solves window by window: shooting_grad steps onto every save"))
    haskey(ERK_NAMES, sname) || throw(ArgumentError("native_solver_train_step drives Euler(), Tsit5(), Heun(), Midpoint(), Ralston(), RK4(), BS3() and DP5(); got $(strategy.solver)"))
    tsteps = (strategy.tstart):(strategy.dt):(strategy.tstop)
    sargs = hasproperty(strategy, :solargs) ? strategy.solargs : (;)
    by_tableau = !(sname in (:Euler, :Tsit5))      # mgn_solver_grad_erk: fixed steps only
    by_tableau && sname in ERK_EMBEDDED && get(sargs, :adaptive, true) != false &&
        throw(ArgumentError("native_solver_train_step trains $(sname)() with fixed steps: pass adaptive = false and dt in the strategy's solargs"))
    by_tableau && batched && throw(ArgumentError("batched = true (shooting_grad) drives Euler() and Tsit5()"))
    adaptive = sname == :Tsit5 && get(sargs, :adaptive, true) != false
    dt = haskey(sargs, :dt) ? sargs[:dt] : (adaptive ? zero(strategy.dt) : strategy.dt)
    abstol = Float32(get(sargs, :abstol, 1e-6)); reltol = Float32(get(sargs, :reltol, 1e-3))
    im = inflow_mask_row === nothing ? nothing : inflow_data
    function window(x0, g, t0, t1, saves; kw...)
        sname == :Euler && return solver_grad(mgn, x0, node_type_onehot, edge_features, val_mask_row, inflow_mask_row, im, g, t0, t1, dt, saves; kw...)
        if by_tableau
            gs, loss, pred, _, _ = solver_grad_erk(sname, mgn, x0, node_type_onehot, edge_features, val_mask_row, inflow_mask_row, im, g, t0, t1, dt, saves; kw...)
            return gs, loss, pred
        end
        gs, loss, pred, _, _ = solver_grad_tsit5(mgn, x0, node_type_onehot, edge_features, val_mask_row, inflow_mask_row, im, g, t0, t1, saves;
            dt = dt, adaptive = adaptive, dense_saves = dense_saves, abstol = abstol, reltol = reltol, kw...)
        return gs, loss, pred
    end
    if !hasproperty(strategy, :interval_size)      # SolverTraining
        gs, loss, _ = window(gt[:, :, 1], gt, strategy.tstart, strategy.tstop, tsteps; loss_scale = n_scale)
        return (gs,), loss
    end
    T = length(tsteps)
    ranges = [i:min(T, i + strategy.interval_size - 1) for i in 1:(strategy.interval_size - 1):(T - 1)]
    if batched && !adaptive
        gs, loss, _ = shooting_grad(mgn, node_type_onehot, edge_features, val_mask_row, inflow_mask_row, im, gt, ranges, tsteps,
            sname == :Euler ? dt : (dt == 0 ? strategy.dt : dt); solver = sname, cont_weight = Float32(strategy.continuity_term))
        return (gs,), loss
    end
    gs_sum = zeros(Float64, length(mgn.ps)); loss_sum = 0.0
    for (i, rg) in enumerate(ranges)
        last_window = i == length(ranges)
        ct = last_window ? nothing : gt[:, :, first(ranges[i + 1])]
        gs, loss, _ = window(gt[:, :, first(rg)], gt[:, :, rg], tsteps[first(rg)], tsteps[last(rg)], tsteps[rg];
            cont_target = ct, cont_weight = last_window ? 0.0f0 : Float32(strategy.continuity_term))
        gs_sum .+= gs; loss_sum += loss
    end
    return (Float32.(gs_sum),), Float32(loss_sum)
end

"""
    rollout_eval(solver, mgn, x0, node_type_onehot, edge_features, val_mask_row, inflow_mask_row, inflow_data, gt, start, stop, dt, saves;
                 sel = nothing, want_pred = false) -> (val_loss, mse_save, mse_time, pred, sol_t)

`native_rollout` with the errors against `gt` (O x N x frames, at least `length(saves)` of them) reduced on the device
(mgn_rollout_eval): `mse_time = mean((prediction - gt) .^ 2; dims = 3)` (O x N, `_validation_step`'s `error`), `mse_save =
mean(...; dims = 2)` (O x saves, `eval_network!`'s `error[:, 1, :]`, Float64) and `val_loss = mean(mse_time[sel])` -- `sel` a vector
of 1-based LINEAR indices into the O x N matrix, exactly what `error[mask]` does with the reference's vector of node indices
(`nothing`: all elements).  Without `want_pred` the solution is neither kept on the device nor downloaded (`pred === nothing`).  Pass
the same array as `gt` and `inflow_data` (validation: the ground truth is the inflow data) and it is uploaded once.  `solver` (the
tableau names included, through mgn_rollout_eval_erk) and `fixed_step`: as `native_rollout`'s.
"""
function rollout_eval(solver, mgn::GraphNetwork, x0::Matrix{Float32}, node_type_onehot::Matrix{Float32}, edge_features::Matrix{Float32},
        val_mask_row::Union{Nothing, Vector{Float32}}, inflow_mask_row::Union{Nothing, Vector{UInt8}},
        inflow_data::Union{Nothing, Array{Float32, 3}}, gt::Array{Float32, 3}, start, stop, dt, saves;
        sel::Union{Nothing, Vector{Int32}} = nothing, want_pred = false, abstol = 1.0f-6, reltol = 1.0f-3, tolerant_inflow = false,
        fixed_step = false)
    name = solver isa Symbol ? solver : nameof(typeof(solver))
    haskey(ERK_NAMES, name) || throw(ArgumentError("rollout_eval drives Euler, Tsit5, Heun, Midpoint, Ralston, RK4, BS3 and DP5; got $name"))
    erk = erk_route(name)
    sync_params!(mgn, mgn.ps::Vector{Float32})
    O, N = size(x0)
    ns = length(saves)
    out = want_pred ? Array{Float32, 3}(undef, O, N, ns) : nothing
    mse_save = Matrix{Float64}(undef, O, ns)
    mse_time = Matrix{Float32}(undef, O, N)
    sdt = ns > 1 ? saves[2] - saves[1] : one(eltype(saves))
    f64 = eltype(saves) == Float64
    d = MgnRolloutDesc(name == :Euler ? 0 : (fixed_step ? 2 : 1), start, stop, dt === nothing ? 0 : dt, sdt, ns, abstol, reltol,
        pointer(x0), pointer(node_type_onehot), pointer(edge_features), opt_ptr(val_mask_row),
        inflow_mask_row === nothing ? Ptr{UInt8}(C_NULL) : pointer(inflow_mask_row), inflow_data === nothing ? Ptr{Float32}(C_NULL) : pointer(inflow_data),
        inflow_data === nothing ? 0 : size(inflow_data, 3), out === nothing ? Ptr{Float32}(C_NULL) : pointer(out), 0, 0, 0,
        tolerant_inflow ? 1 : 0, f64 ? 1 : 0, start, stop, dt === nothing ? 0 : dt, sdt)
    e = MgnRolloutEvalDesc(pointer(gt), size(gt, 3), pointer(mse_save), pointer(mse_time), sel === nothing ? Ptr{Int32}(C_NULL) : pointer(sel),
        sel === nothing ? 0 : length(sel), 1, 0.0)
    # (@ccall: tests/test_rollout_eval_host.py checks this call against the header)
    rc = if erk === nothing
        GC.@preserve x0 node_type_onehot edge_features val_mask_row inflow_mask_row inflow_data out gt mse_save mse_time sel @ccall LIB.mgn_rollout_eval(
            mgn.handle::Ptr{Cvoid}, d::Ref{MgnRolloutDesc}, e::Ref{MgnRolloutEvalDesc})::Cint
    else      # (d.solver is not read)
        adaptive = erk_adaptive(name, dt, fixed_step)
        GC.@preserve x0 node_type_onehot edge_features val_mask_row inflow_mask_row inflow_data out gt mse_save mse_time sel erk @ccall LIB.mgn_rollout_eval_erk(
            mgn.handle::Ptr{Cvoid}, d::Ref{MgnRolloutDesc}, e::Ref{MgnRolloutEvalDesc}, erk::Ptr{Float64}, adaptive::Int32)::Cint
    end
    check(mgn.handle, rc)
    return e.val_loss, mse_save, mse_time, out, collect(saves)
end

"""
    native_validation_step(strategy, mgn, gt, node_type_onehot, edge_features, mask, val_mask_row, inflow_mask_row, solver, solver_dt;
                           want_arrays = false) -> (loss, gt, prediction)

`validation_step(strategy, t)` (src/strategies.jl:111-134 through every strategy's method; called at src/MeshGraphNets.jl:433) in
one native call: the rollout from `gt[:, :, 1]` over the strategy's interval (`tstart:dt:tstop`; a strategy without one passes
`sim_interval`), `error = mean((prediction - gt) .^ 2; dims = 3)` and `mean(error[mask])` on the device -- `mask` the reference's
`Int32.(findall(...))`, indexing the matrix linearly as there.  `gt` (O x N x frames: `vcat` of the target fields) is the inflow data
too.  The last two results are `nothing` unless `want_arrays` (train_mgn! keeps them for the first trajectory only).  `fixed_step =
true` with a `solver_dt` is the reference's own call (`_validation_step` hands `solver_valid_dt` to `rollout`'s `adaptive = false`
branch); the default keeps the results this function has always returned.
"""
function native_validation_step(strategy, mgn::GraphNetwork, gt::Array{Float32, 3}, node_type_onehot::Matrix{Float32},
        edge_features::Matrix{Float32}, mask::Vector{Int32}, val_mask_row::Union{Nothing, Vector{Float32}},
        inflow_mask_row::Union{Nothing, Vector{UInt8}}, solver, solver_dt;
        sim_interval = (strategy.tstart):(strategy.dt):(strategy.tstop), want_arrays = false, fixed_step = false)
    ns = length(sim_interval)
    loss, _, _, pred, _ = rollout_eval(solver, mgn, gt[:, :, 1], node_type_onehot, edge_features, val_mask_row, inflow_mask_row,
        inflow_mask_row === nothing ? nothing : gt, gt, sim_interval[1], sim_interval[end], solver_dt, sim_interval;
        sel = mask, want_pred = want_arrays, fixed_step = fixed_step && solver_dt !== nothing)
    return Float32(loss), want_arrays ? gt[:, :, 1:ns] : nothing, pred
end

# ---- multi-GPU: one Julia process per GPU (e.g. under MPI.jl or Distributed), one handle each; the halo exchange (RCCL grouped
# send / recv over xGMI) and the overlap schedule run inside the library.  With `nranks > 1` and a communicator,
# `mgn.model(graph, ps, st)` takes the GLOBAL FeatureGraph on every rank and returns the complete output on every rank.
const COMM_ID_BYTES = 128
const COMM_RCCL = Int32(0)
const COMM_HOST = Int32(1)      # shared memory on one node (several ranks on one GPU; tests)
const COMM_LOCAL = Int32(2)     # the ranks are threads (tasks on distinct threads) of THIS process; device rows stay on the device

"Made on ONE rank; distribute the bytes to the others (`MPI.Bcast!(id, 0, comm)`), then every rank calls `comm_init!`."
function comm_unique_id(transport::Int32 = COMM_RCCL)
    id = Vector{UInt8}(undef, COMM_ID_BYTES)
    rc = ccall((:mgn_comm_unique_id, LIB), Cint, (Ptr{UInt8}, Int32), id, transport)
    rc == 0 || error(unsafe_string(ccall((:mgn_last_error, LIB), Cstring, (Ptr{Cvoid},), C_NULL)))
    return id
end

function comm_init!(mgn::GraphNetwork, id::Vector{UInt8}, transport::Int32 = COMM_RCCL)
    GC.@preserve id check(mgn.handle,
        ccall((:mgn_comm_init, LIB), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Csize_t, Int32), mgn.handle, id, length(id), transport))
    return mgn
end

"Bootstrap without MPI: rank 0 writes the id to `path` (a filesystem every rank sees), the others wait for it."
comm_init_file!(mgn::GraphNetwork, path::AbstractString, transport::Int32 = COMM_RCCL) =
    (check(mgn.handle, ccall((:mgn_comm_init_file, LIB), Cint, (Ptr{Cvoid}, Cstring, Int32), mgn.handle, path, transport)); mgn)

comm_barrier(mgn::GraphNetwork) = check(mgn.handle, ccall((:mgn_comm_barrier, LIB), Cint, (Ptr{Cvoid},), mgn.handle))

"`nsteps` processor steps on the engine-resident latents (the benchmarked unit); every rank calls it."
processor_steps_dev!(mgn::GraphNetwork, nsteps::Integer) =
    check(mgn.handle, ccall((:mgn_processor_steps_dev, LIB), Cint, (Ptr{Cvoid}, Int32), mgn.handle, nsteps))

end # module
