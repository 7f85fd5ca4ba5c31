/*
 * mgn_hip.h -- C ABI of the MI355X-native MeshGraphNets Encode-Process-Decode engine.
 *
 * This is the drop-in boundary for the ONE hot path of una-auxme/MeshGraphNets.jl: everything the
 * reference obtains from `using GraphNetCore` (reference src/MeshGraphNets.jl:8) that runs per
 * ODE right-hand side / per training datapoint.  A thin Julia `ccall` shim (julia/MGNHip.jl) or the
 * Python ctypes host (meshgraphnets.jl_amd/engine.py) binds exactly these symbols; see
 * INTEGRATION.md.  No C++ types, no torch types: plain pointers and sizes.
 *
 * Conventions
 *   - All matrices are C row-major [count][feat] == the bytes of Julia's column-major (feat x count).
 *   - Every function returns 0 (MGN_OK) or a negative mgn_status; text via mgn_last_error().
 *   - A handle is NOT thread-safe; one in-flight call per handle (the reference calls the model
 *     strictly sequentially from one task: ODE RHS inside `solve`, src/solve.jl:53-61).
 *   - Host-pointer entry points copy in/out and return after the D2H copy; `_dev` entry points take
 *     device pointers, enqueue on the handle's stream (mgn_set_stream) and do not synchronise.
 *   - The engine owns all device memory it allocates; caller owns every buffer it passes in.
 *   - There is no CPU fallback: without a HIP device every compute entry point fails with MGN_E_HIP.
 */
#ifndef MGN_HIP_H
#define MGN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum mgn_status {
    MGN_OK = 0,
    MGN_E_ARG = -1,   /* bad argument (reference: ArgumentError / DimensionMismatch)            */
    MGN_E_HIP = -2,   /* HIP runtime error / no device                                          */
    MGN_E_STATE = -3, /* call order violated (e.g. forward before set_params / set_graph)       */
    MGN_E_OOM = -4,   /* device or host allocation failed                                       */
    MGN_E_UNSUPPORTED = -5,
    MGN_E_RCCL = -6   /* communicator: RCCL error, peer time-out, exchange before mgn_comm_init              */
} mgn_status;

typedef enum mgn_dtype { MGN_F32 = 0, MGN_BF16 = 1 } mgn_dtype;

/* Mirrors the arguments of GraphNetCore.load(quantities, dims, e_norms, n_norms, o_norms, outputs,
 * mps, layer_size, hidden_layers, opt, device, path) at reference src/MeshGraphNets.jl:282-285:
 *   Fn = quantities, Fe = dims+1 (src/graph.jl:49-52), O = outputs, L = layer_size.            */
typedef struct mgn_config {
    int32_t Fn;            /* node input width  (cylinder_flow: 9 = velocity 2 + one-hot 7)       */
    int32_t Fe;            /* edge input width  (2-D mesh: 3 = rel pos 2 + norm)                  */
    int32_t O;             /* output width      (cylinder_flow: 2)                                */
    int32_t L;             /* latent width `layer_size`; HIP path supports 32, 64, 128            */
    int32_t hidden_layers; /* hidden layers per MLP (h + 1 Dense): 1 .. 4.  2 (the example's value) runs the tuned kernel */
                           /* families; other counts run the general instantiations (mgn_step / mgn_ode_vjp /      */
                           /* mgn_forward_vjp follow it too; MGN_BF16 is specialised for 2 and refuses others)     */
    int32_t mps;           /* message passing steps                                               */
    int32_t dtype;         /* mgn_dtype: MGN_F32, or MGN_BF16 (L = 128: bf16 storage + bf16 MFMA in the processor, */
                           /* fp32 accumulate / LayerNorm / residual / aggregation; encoder, decoder in fp32)      */
    int32_t rank;          /* this process's partition, 0 <= rank < nranks                        */
    int32_t nranks;        /* number of edge-cut partitions (1 = whole mesh on this GPU)          */
    int32_t device;        /* HIP device ordinal, -1 = current device, MGN_DEVICE_NONE = host-only handle */
    int32_t n_edge_sets;   /* 0 or 1: the reference's single edge set (FeatureGraph, src/graph.jl:87-96);          */
                           /* 2: mesh edges + world edges (MGN-spec "per edge set"; flag_simple-shaped, BASELINE cfg-3) */
    int32_t Fe2;           /* edge input width of the second set (used when n_edge_sets == 2)                      */
    int32_t ln_mode;       /* mgn_ln_mode: which LayerNorm GraphNetCore / Lux compute (the sources are not vendored:     */
                           /* julia/spec_probe.jl tells).  MGN_LN_VAR_EPS (0, MGN-spec v1): (x - mean) / sqrt(var + eps);  */
                           /* MGN_LN_STD_EPS: (x - mean) / (sqrt(var) + eps).  eps = 1e-5, biased variance, per row.       */
                           /* Every entry point follows it, the reverse passes (mgn_step, mgn_forward_vjp, mgn_ode_vjp) included */
    int32_t ln_dims;       /* mgn_ln_dims: MGN_LN_ROWS (0, MGN-spec v1): LayerNorm statistics per node / edge over its L features.   */
                           /* MGN_LN_ALL: over the WHOLE (L x rows) array of an MLP's output -- what Lux 0.5's LayerNorm(shape) computes  */
                           /* when it is left at dims = Colon() (julia/spec_probe.jl tells which one the installed GraphNetCore / Lux    */
                           /* run).  A different network, not a numerical variant: every LayerNorm then couples all rows, so the fused    */
                           /* tile kernels cannot be used; the mode runs unfused (MLP kernel with its LayerNorm off, grid-wide statistics    */
                           /* in double, apply pass) behind mgn_forward, mgn_processor_steps, mgn_set_static + mgn_ode_step (both forms),   */
                           /* mgn_rollout, mgn_processor_steps_dev (the resident latents pass through the same driver as rows), and in     */
                           /* both directions behind mgn_step, mgn_forward_vjp, mgn_ode_vjp: fp32, one partition, one edge set.  The staged */
                           /* per-step calls of the fused kernels (mgn_proc_*, mgn_fwd_*) answer MGN_E_UNSUPPORTED                          */
    /* Widths.  Fn, Fe, Fe2, O >= 1.  The inference entry points on ln_dims = MGN_LN_ROWS (mgn_forward, mgn_ode_step, mgn_set_static,   */
    /* mgn_rollout*, mgn_rollout_eval*, the staged mgn_fwd_* calls) serve ANY width: the first layers read their inputs feature by     */
    /* feature, the decoder writes its O columns one by one.  Everything that computes on the training kernels needs                   */
    /* Fn, Fe, Fe2, O <= L -- they pad every input to L columns and hold the decoder's output in rows of L: the training entry points  */
    /* (mgn_step, mgn_step_datapoint(s) and the mgn_train_* / mgn_datapoint_export calls around them, mgn_ode_vjp, mgn_forward_vjp,     */
    /* mgn_solver_grad, mgn_solver_grad_tsit5, mgn_solver_grad_erk, mgn_shooting_grad, their mgn_group_* forms) answer                 */
    /* MGN_E_UNSUPPORTED naming the width and L, before the device check (a MGN_DEVICE_NONE handle answers it too), any allocation,   */
    /* launch or collective; the handle stays usable.  ln_dims = MGN_LN_ALL runs ALL of its compute on those kernels, inference        */
    /* included: mgn_create answers MGN_E_ARG for such a configuration with a width above L.                                          */
} mgn_config;

typedef enum { MGN_LN_VAR_EPS = 0, MGN_LN_STD_EPS = 1 } mgn_ln_mode;
typedef enum { MGN_LN_ROWS = 0, MGN_LN_ALL = 1 } mgn_ln_dims;

#define MGN_MAX_EDGE_SETS 2

/* A handle created with device == MGN_DEVICE_NONE owns no GPU state: only mgn_set_graph and the partition
 * introspection calls work on it (host logic: receiver sort, CSR, edge-cut partition, halo lists); every
 * compute entry point returns MGN_E_HIP.  It exists so that the partitioner can be used and tested on
 * hosts without a GPU; it is not a CPU compute path. */
#define MGN_DEVICE_NONE (-2)

typedef struct mgn_engine mgn_handle;

/* ---- lifecycle ------------------------------------------------------------------------------ */
/* Version of THIS header's structs and prototypes; bumped whenever mgn_config / mgn_rollout_desc grow or a prototype changes.  A
 * binding compiled against another version must not call in (a shorter mgn_config would be read past its end): the Python and
 * Julia bindings compare mgn_abi_version() with the constant they were written for before the first mgn_create. */
#define MGN_ABI_VERSION 4
int mgn_abi_version(void);
int mgn_create(const mgn_config* cfg, mgn_handle** out);
void mgn_destroy(mgn_handle* h);
const char* mgn_last_error(const mgn_handle* h); /* h may be NULL: error of the last failed mgn_create */
/* Stream all work of the handle is enqueued on.  hip_stream is a hipStream_t; NULL is HIP's default (null)
 * stream -- what torch.cuda.current_stream().cuda_stream returns for torch's default stream -- and
 * MGN_STREAM_OWN selects the engine's private non-blocking stream (the state after mgn_create).  Callers that
 * mix engine calls with other GPU work (RCCL collectives, torch copies) must pass THEIR stream here. */
#define MGN_STREAM_OWN ((void*)(intptr_t)-1)
int mgn_set_stream(mgn_handle* h, void* hip_stream);
int mgn_synchronize(mgn_handle* h);

/* ---- parameters: mgn.ps (reference src/MeshGraphNets.jl:288,376-377) ------------------------- */
/* Packed order (MGN-spec v1): enc-node, enc-edge, step1-edge, step1-node, ..., decoder;
 * within an MLP W1,b1,W2,b2,W3,b3,[ln_scale,ln_bias]; each W row-major [in][out].
 * mgn_set_params copies the vector (0.1 ms for the 15-step model) and is meant to be called whenever the caller's
 * parameters MAY have changed -- the reference's loop updates them before every step! (src/MeshGraphNets.jl:375-377):
 * values equal to the ones held invalidate nothing; new ones are turned into the kernels' layouts on the device by the
 * next call that computes with them (1.5 ms for the inference kernels, 0.4 ms inside mgn_step).
 * The handle keeps two copies of the vector, one on the host and one resident on the device, and knows which is
 * authoritative: after mgn_set_params the host copy (the device copy follows at the next pack), after
 * mgn_set_params_dev / mgn_adam_update the device copy (mgn_get_params, the inference layouts and the debug checks
 * refresh the host copy first: one copy and one synchronisation, only when it is stale).  The "same values again"
 * shortcut of mgn_set_params is taken only while the host copy is current.                                     */
size_t mgn_param_count(const mgn_config* cfg);
int mgn_set_params(mgn_handle* h, const float* packed, size_t n);
int mgn_get_params(mgn_handle* h, float* packed, size_t n);

/* ---- parameters that stay on the device; Optimisers.Adam there (reference src/MeshGraphNets.jl:288,375-377) ----
 * mgn_step / mgn_step_datapoint(s) leave the gradient in device memory; these calls are the way back, so that one
 * iteration of the reference's loop -- gs = step!(...); opt_state, ps = Optimisers.update(opt_state, ps, gs) -- is two
 * calls with nothing of parameter size crossing PCIe.  The loop stays the caller's.
 *
 * mgn_set_params_dev: packed [n = mgn_param_count] (host or device pointer) is copied into the resident vector with
 * hipMemcpyDefault on the handle's stream.  It always counts as a change: nothing is compared, and it invalidates
 * exactly what mgn_set_params does (training layouts, inference layouts, captured inference graphs, the static RHS
 * cache).  With a device source there is no host work and no synchronisation (a captured inference graph, where one
 * exists, is waited for before it is destroyed); a host source has left the caller's memory on return.  The next
 * training call re-packs its weights with a memset and the pack launches alone: the chunk list and the description of
 * the bias / LayerNorm tables depend on the configuration only and stay on the device.
 * mgn_get_params_dev: the parameters as they stand into packed (host or device pointer); blocks for a host one.
 *
 * mgn_adam_init (Optimisers.setup(Optimisers.Adam(eta, (beta1, beta2), epsilon), ps)): mt = vt = 0, beta_t = (beta1,
 * beta2); calling it again resets the state.  mgn_set_params* do not touch it, a new graph keeps it, mgn_destroy
 * frees it.
 * mgn_adam_update (Optimisers.update): one launch over the resident vector, per element in fp32 with every
 * operation rounded once and nothing contracted:
 *     m <- b1 m + (1 - b1) g      v <- b2 v + (1 - b2) (g g)      p <- p - ((m / c1) / (sqrt(v / c2) + eps)) eta
 * with c_i = (float)(1 - beta_t[i]) formed from the double beta_t, then beta_t[i] *= beta_i in double -- the order of
 * operations of Optimisers.Adam (and of checkpoint.Adam.update, its Python twin).  grads [n_grads = mgn_param_count]
 * host or device; a device gradient adds no copy and no synchronisation.  Invalidates as mgn_set_params_dev does.
 * g g that overflows or is subnormal is not specified.
 * mgn_adam_state, the checkpoint hook: write = 0 copies mt, vt ([mgn_param_count] each, host or device) and beta_t
 * out, write = 1 in (the descriptor of mgn_adam_init stays); blocks where a pointer is host memory.
 *
 * Any dtype, any ln_mode / ln_dims; rank handles of a partitioned mesh take all five calls (every rank holds the whole
 * vector and mgn_step hands every rank the same gradient bits, so the ranks stay in step).  Refusals, all before any
 * launch, the handle stays usable.  MGN_E_ARG: NULL pointers, n != mgn_param_count, write other than 0 / 1, a
 * descriptor that is not finite or outside eta > 0, 0 <= beta < 1, epsilon > 0.  MGN_E_HIP: a host-only handle.
 * MGN_E_STATE: mgn_adam_update / mgn_adam_state before mgn_adam_init, mgn_adam_update / mgn_get_params_dev before
 * any parameters were set.                                                                                      */
int mgn_set_params_dev(mgn_handle* h, const float* packed, size_t n);
int mgn_get_params_dev(mgn_handle* h, float* packed, size_t n);
typedef struct mgn_adam_desc { float eta, beta1, beta2, epsilon; } mgn_adam_desc;
int mgn_adam_init(mgn_handle* h, const mgn_adam_desc* a);
int mgn_adam_update(mgn_handle* h, const float* grads, size_t n_grads);
int mgn_adam_state(mgn_handle* h, int32_t write, float* mt, float* vt, double beta_t[2]);

/* ---- normalisers: mgn.n_norm / e_norm / o_norm frozen to per-feature affine maps --------------
 * forward:  y = x*scale + shift  (covers NormaliserOfflineMinMax, OfflineMeanStd and a frozen
 * NormaliserOnline; reference src/MeshGraphNets.jl:79-203, applied src/graph.jl:80-93);
 * inverse_data(o_norm, y) = y*out_scale + out_shift (src/solve.jl:205-210).
 * Any pointer may be NULL = identity.  Used by mgn_ode_step only.                                */
int mgn_set_norms(mgn_handle* h, const float* node_scale, const float* node_shift, /* [Fn] */
                  const float* edge_scale, const float* edge_shift,               /* [Fe] */
                  const float* out_scale, const float* out_shift);                /* [O]  */

/* ---- graph: once per trajectory, like create_base_graph (reference src/graph.jl:25-55, called at
 * src/MeshGraphNets.jl:360,418,596).  Sort-by-receiver, CSR, tiling and (nranks>1) the edge-cut
 * partition + halo lists are built here.  index_base is 1 at the Julia boundary (src/graph.jl:31-34).
 * mesh_pos [N][pos_dim] is optional; it drives the geometric partition when nranks > 1.         */
int mgn_set_graph(mgn_handle* h, int32_t N, int64_t E, const int32_t* senders, const int32_t* receivers,
                  int32_t index_base, const float* mesh_pos, int32_t pos_dim);

/* Rank-local ingest of the same graph (nranks > 1 at scale: mgn_set_graph walks the GLOBAL edge lists on every rank).
 * mgn_partition_nodes: the node partition mgn_set_graph would derive -- recursive coordinate bisection of mesh_pos [N][pos_dim], or
 * contiguous index blocks when mesh_pos is NULL -- as owner[N]; deterministic, no handle needed, every rank gets the same map.
 * mgn_set_graph_local: rank h->cfg.rank hands over only the edges it has an END of (sender or receiver owned; the others concern
 * neither its tiles nor its send lists), in the order of the global list, with their positions edge_gid[E_touch] (ascending) in that
 * list of E_global edges.  The handle ends up in exactly the state mgn_set_graph(N, E_global, ...) with the same partition leaves it
 * in (tests/test_abi_and_host.py); arrays indexed by edge at the boundary ([E][Fe] inputs, latents) stay GLOBAL arrays, of which the
 * rank touches the rows of its local edges.  One edge set; index_base as in mgn_set_graph.                                          */
int mgn_partition_nodes(int32_t N, const float* mesh_pos, int32_t pos_dim, int32_t nranks, int32_t* owner);
int mgn_set_graph_local(mgn_handle* h, int32_t N, const int32_t* owner, int64_t E_global, int64_t E_touch, const int32_t* senders,
                        const int32_t* receivers, const int64_t* edge_gid, int32_t index_base);

/* Second edge set (n_edge_sets == 2): topology of set `set` (>= 1) over the same N nodes, after mgn_set_graph and
 * as often as it changes (world edges are re-searched every step of a cloth rollout; the mesh set, the node
 * partition and the node order stay).  Edges live with their receiver's owner like mesh edges; with nranks > 1
 * the halo / send lists become the union over the sets, so query mgn_halo_* again afterwards.  E may be 0.
 * The reference has one edge set; this is the MGN-spec extension SURVEY.md 8c defines (GOLD-C).                */
int mgn_set_edge_set(mgn_handle* h, int32_t set, int64_t E, const int32_t* senders, const int32_t* receivers,
                     int32_t index_base);
/* Raw features [E_set][Fe2] of set >= 1 for the next mgn_forward / mgn_fwd_upload (which carry set 0's `ef`).
 * No normaliser is applied to them (normalise on the host, or fold the affine map into the first layer).       */
int mgn_set_edge_features(mgn_handle* h, int32_t set, const float* ef);
int mgn_edge_set_info(const mgn_handle* h, int32_t set, int64_t* E, int64_t* e_local);
/* Latents of edge set `set` (0 included), host GLOBAL arrays [E_set][L]; mgn_latents_import/export cover v and set 0. */
int mgn_edge_latents_import(mgn_handle* h, int32_t set, const float* e);
int mgn_edge_latents_export(mgn_handle* h, int32_t set, float* e);

/* Partition introspection (nranks == 1: n_own = N, n_halo = 0, e_local = E). */
int mgn_partition_info(const mgn_handle* h, int32_t* n_own, int32_t* n_halo, int64_t* e_local);
int mgn_owned_nodes(const mgn_handle* h, int32_t* global_ids /* [n_own], 0-based */);
int mgn_local_edges(const mgn_handle* h, int64_t* global_edge_ids /* [e_local], engine order */);
int mgn_halo_counts(const mgn_handle* h, int32_t* send_rows /* [nranks] */, int32_t* recv_rows /* [nranks] */);
int mgn_halo_nodes(const mgn_handle* h, int32_t* global_ids /* [n_halo], grouped by owner rank */);
int mgn_halo_send_index(const mgn_handle* h, int32_t* local_rows /* [sum(send_rows)] owned local rows, peer-major */);
/* local (receiver-sorted) edge list: snd may index halo rows (>= n_own); rowptr is CSR by receiver */
int mgn_local_graph(const mgn_handle* h, int32_t* snd /* [e_local] */, int32_t* rcv /* [e_local] */, int32_t* rowptr /* [n_own+1] */);
int mgn_node_owner(const mgn_handle* h, int32_t* owner /* [N] rank owning each global node */);
/* owned nodes are numbered boundary-first: local rows [0, n_boundary) are the nodes some peer lists as halo */
int mgn_boundary_count(const mgn_handle* h, int32_t* n_boundary);

/* ---- the model: mgn.model(graph, ps, st) -> output (reference src/solve.jl:200) ---------------
 * nf [N][Fn], ef [E][Fe] are the FeatureGraph fields (already normalised, src/graph.jl:87-96);
 * out [N][O].  With nranks > 1 every rank passes the GLOBAL arrays (each uploads only the rows it owns) and, after
 * mgn_comm_init, receives the complete GLOBAL output (owned rows are gathered over the communicator).           */
int mgn_forward(mgn_handle* h, const float* nf, const float* ef, float* out);

/* ---- the fused RHS: ode_step (reference src/solve.jl:188-219) incl. build_graph (src/graph.jl:75-97)
 * x [N][O] state, node_type_onehot [N][Fn-O] (raw), ef_raw [E][Fe] (raw edge_features),
 * val_mask [N] (0/1; reference repeats it over the O rows, src/MeshGraphNets.jl:588-591), may be NULL.
 * dxdt [N][O] = inverse_data(o_norm, model(graph)) .* val_mask.                                 */
int mgn_ode_step(mgn_handle* h, const float* x, const float* node_type_onehot, const float* ef_raw,
                 const float* val_mask, float* dxdt);

/* Static per-trajectory inputs of the RHS, set ONCE (like create_base_graph's outputs, reference src/graph.jl:54):
 * node_type_onehot [N][Fn-O], ef_raw [E][Fe], val_mask [N] or NULL.  They are uploaded once, the edge encoder runs
 * once and its output is cached; afterwards mgn_ode_step may be called with node_type_onehot = ef_raw = val_mask =
 * NULL and only moves the O x N state per call (on small meshes it replays a hipGraph of the launch sequence).
 * Invalidated by mgn_set_params / mgn_set_norms / mgn_set_graph. */
int mgn_set_static(mgn_handle* h, const float* node_type_onehot, const float* ef_raw, const float* val_mask);

/* ---- graph prologue helpers (GraphNetCore utilities used at reference src/graph.jl:26-52) -------
 * Scalable replacements for the reference's per-edge host loops (which cannot build a 6 M-edge graph).
 * No handle, no GPU needed.
 * mgn_triangles_to_edges: cells [C][3] (any index base) -> unique undirected edges, returned two-way
 *   (senders = [a;b], receivers = [b;a], a = max, b = min) in first-occurrence order like the reference.
 *   Call with senders = receivers = NULL to get the count; *n_directed receives 2 x (unique undirected edges).
 * mgn_edge_features: ef[e] = [pos[s]-pos[r] ; ||pos[s]-pos[r]||]  (src/graph.jl:35-36,49-52), ef is [E][dim+1]. */
int mgn_triangles_to_edges(const int32_t* cells, int64_t n_cells, int32_t* senders, int32_t* receivers, int64_t* n_directed);
/* World edges of a cloth-like mesh (second edge set of MGN-spec; no reference symbol, the reference has one edge set):
 * every ordered pair (s, r), s != r, closer than `radius` in world space and not already joined by a mesh edge; uniform
 * grid search, receiver-major output with ascending senders.  Call with senders = receivers = NULL to get the count in
 * *n_edges; with buffers, *n_edges holds their capacity on entry and the number written on return.               */
int mgn_world_edges(const float* world_pos, int32_t dim, int32_t N, float radius, const int32_t* mesh_senders,
                    const int32_t* mesh_receivers, int64_t n_mesh, int32_t index_base, int32_t* senders, int32_t* receivers,
                    int64_t* n_edges);
int mgn_edge_features(const float* mesh_pos, int32_t pos_dim, const int32_t* senders, const int32_t* receivers,
                      int64_t E, int32_t index_base, float* ef);

/* The same prologue ON THE DEVICE: the reference's per-edge host loops cannot build a 6 M-edge graph.
 * Integer results are bit-identical to the host versions above (same packed (max, min) keys, stable radix sort, first-occurrence
 * order restored by a second sort).  Pointers may be host or device memory (hipMemcpyDefault).
 * mgn_triangles_to_edges_dev: as mgn_triangles_to_edges; `capacity` = entries of each output buffer (6 x n_cells always suffices);
 *   MGN_E_ARG with *n_directed set when they are too small.
 * mgn_set_static_mesh: create_base_graph's FEATURE half (src/graph.jl:26-27,35-36,49-52) into the engine's resident static inputs:
 *   one_hot(node_type, depth = type_max - type_min + 1, offset = 1 - type_min) and edge_features = [mesh_pos[s] - mesh_pos[r]; norm]
 *   are computed by kernels in engine order -- no [E][Fe] host array, no PCIe transfer of it -- then the edge encoder runs once, as
 *   in mgn_set_static; afterwards mgn_ode_step(x, NULL, NULL, NULL) / the resident fast path apply.  Needs Fn - O == depth, Fe == pos_dim + 1.
 *   A node whose type lies outside [type_min, type_max] gets a one-hot row of zeros (no error; the reference's one_hot would throw).
 * mgn_world_edges_dev: the world-edge set `set` (>= 1) of a cloth-like mesh searched on the device (uniform grid, radix sort by cell)
 *   and installed WITHOUT a host round trip (what mgn_world_edges + mgn_set_edge_set do on the host; cloth rollouts re-search every
 *   step); with Fe2 == dim + 1 its features [rel world pos; norm] are written too.  One partition.  The same edges as
 *   mgn_world_edges, receiver-major with ascending senders IN THE ENGINE'S NODE NUMBERING: on a handle that mgn_set_graph did not
 *   renumber that is mgn_world_edges' order entry for entry; on a renumbered handle (scattered node labels) the same SET of edges,
 *   ordered by the engine's ids (position in mgn_owned_nodes) of receiver, then sender.  mgn_edge_set_export hands the installed lists
 *   back in that order, in the caller's ids (0-based). */
int mgn_triangles_to_edges_dev(mgn_handle* h, const int32_t* cells, int64_t n_cells, int32_t* senders, int32_t* receivers, int64_t capacity,
                               int64_t* n_directed);
int mgn_set_static_mesh(mgn_handle* h, const int32_t* node_type /* [N] */, int32_t type_min, int32_t type_max, const float* mesh_pos /* [N][pos_dim] */,
                        int32_t pos_dim, const float* val_mask /* [N] or NULL */);
int mgn_world_edges_dev(mgn_handle* h, int32_t set, const float* world_pos /* [N][dim] */, int32_t dim, float radius, int64_t* n_edges);
int mgn_edge_set_export(mgn_handle* h, int32_t set, int32_t* senders, int32_t* receivers);

/* Online-normaliser accumulation as a device reduction: what GraphNetCore's NormaliserOnline adds up per call
 * (normalisers built at reference src/MeshGraphNets.jl:92,193-199, applied in build_graph src/graph.jl:75-97):
 * sum[f] = sum_r x[r][f], sum_squares[f] = sum_r x[r][f]^2 over x [rows][dim] (host or device pointer), accumulated in double
 * in a fixed order (bitwise repeatable).  The caller keeps the running totals, count and max_accumulations logic.          */
int mgn_feature_stats(mgn_handle* h, const float* x, int64_t rows, int32_t dim, double* sum, double* sum_squares);

/* ---- native rollout driver: the whole `rollout` of reference src/solve.jl:42-68 on the device:
 * ODEProblem(ode_func_eval, x0, (t0, t1), ...) solved with fixed-step Euler (`adaptive = false, dt = dt`) or an
 * adaptive Tsit5 (own tableau + PI step controller, tstops = saveat = t0 + i*saves_dt), the right-hand side being
 * ode_func_eval (inflow overwrite from `inflow_data[floor(t / saves_dt)]`, src/solve.jl:151-152 -- see inflow_rule --, applied IN PLACE to
 * the array the RHS is evaluated on, like the reference) -> ode_step (mgn_ode_step semantics).  No host round trip
 * per RHS; one small D2H (error norm) per adaptive step.  Normalisers must be set with mgn_set_norms.
 * MGN_SOLVER_TSIT5_FIXED is solve(prob, Tsit5(); adaptive = false, dt = dt, saveat = saves): the time grid, stage times and dense saves
 * of step mode 2 of mgn_solver_grad_tsit5 (below; the same time loop runs both), in the evaluation form -- the state, the stage inputs
 * and x_{n+1} each take, in place, the inflow rows of the frame of the time their stage sees (stage sum and rows are one launch); save 0
 * is x0 untouched.  dt <= 0 is MGN_E_ARG before any launch; abstol / reltol are ignored.  No error norm: no D2H and, on partitions, no
 * reduction per step.  On return n_accept is the number of steps, n_reject 0, n_rhs = 1 + 6 n_accept.
 * A solver value outside 0 .. 2 is MGN_E_ARG.
 * With nranks > 1 (after mgn_comm_init) every rank passes the GLOBAL arrays and integrates the rows it owns; the error norm of
 * the step controller is reduced over the ranks (the same bits everywhere: the same accept / reject decisions), the halo exchange
 * runs inside every right-hand side, and every rank returns the complete solution.  mgn_ode_step and mgn_set_static likewise
 * (global arrays in, complete dx/dt out on every rank). */
typedef struct mgn_rollout_desc {
    int32_t solver;          /* mgn_solver: 0 = Euler fixed step, 1 = Tsit5 adaptive, 2 = Tsit5 fixed step   */
    float t0, t1;            /* integration interval                                                         */
    float dt;                /* Euler, Tsit5 fixed step: the step (> 0); Tsit5 adaptive: initial step (0 = automatic) */
    float saves_dt;          /* spacing of the save points AND of the inflow_data frames                     */
    int32_t n_saves;         /* solution is stored at t0 + i*saves_dt, i = 0..n_saves-1                      */
    float abstol, reltol;    /* adaptive Tsit5 only (OrdinaryDiffEq defaults: 1e-6, 1e-3); solvers 0 and 2 ignore them */
    const float* x0;               /* [N][O]                                                                 */
    const float* node_type_onehot; /* [N][Fn-O]                                                              */
    const float* ef_raw;           /* [E][Fe]                                                                */
    const float* val_mask;         /* [N] or NULL                                                            */
    const uint8_t* inflow_mask;    /* [N] 0/1 or NULL: rows overwritten from inflow_data                      */
    const float* inflow_data;      /* [n_frames][N][O] or NULL                                               */
    int32_t n_frames;
    float* out;                    /* [n_saves][N][O]                                                        */
    int32_t n_accept, n_reject, n_rhs; /* filled on return                                                   */
    /* Which inflow frame a right-hand side at time t reads.  MGN_INFLOW_REFERENCE (0, the default of a zeroed descriptor): the
     * reference's own expression `floor(Int, t / saves_dt) + 1` (src/solve.jl:151) evaluated in the solver's time type with no
     * tolerance -- so a t an ulp below a frame boundary reads the previous frame, exactly as the reference does (in Float64,
     * 0.29 / 0.01 floors to 28) -- and a frame outside inflow_data is MGN_E_ARG (reference: BoundsError).  MGN_INFLOW_TOLERANT:
     * floor(t / saves_dt + 1e-3) (step k of a fixed-step solve reads frame k whatever its time type), clamped to the frames given.                                                              */
    int32_t inflow_rule;
    /* The solver's time type.  0: Float32, the type of the example's `0.0f0:0.01f0:5.99f0` (examples/cylinder_flow/cylinder_flow.jl:
     * 79-93): t0, t1, dt, saves_dt above are the times, and every time operation is rounded to float.  1: Float64: the four
     * *_f64 fields are the times (a Float64 0.01 is not a float), the float ones are ignored.  The integrator's time advances as
     * OrdinaryDiffEq's does: t <- t + dt per accepted step, the stop's own value when a step ends on a stop.                */
    int32_t time_f64;
    double t0_f64, t1_f64, dt_f64, saves_dt_f64;
} mgn_rollout_desc;
typedef enum mgn_inflow_rule { MGN_INFLOW_REFERENCE = 0, MGN_INFLOW_TOLERANT = 1 } mgn_inflow_rule;
/* mgn_rollout_desc.solver.  The reference's `rollout` branches on dt alone (src/solve.jl:57-61): without dt it is
 * solve(prob, solver; saveat = saves, tstops = saves) -- MGN_SOLVER_TSIT5 --, with dt it is solve(prob, solver; adaptive = false, dt = dt,
 * saveat = saves) whatever the solver -- MGN_SOLVER_EULER, and for Tsit5 (`solver_valid_dt`, `eval_network(...; dt)`) MGN_SOLVER_TSIT5_FIXED.
 * MGN_SOLVER_TSIT5_FIXED is served by mgn_rollout, mgn_rollout_eval and their group forms on every handle that serves MGN_SOLVER_TSIT5;
 * the training entry points answer it as any value they do not know (MGN_E_ARG).                                                      */
typedef enum mgn_solver { MGN_SOLVER_EULER = 0, MGN_SOLVER_TSIT5 = 1, MGN_SOLVER_TSIT5_FIXED = 2 } mgn_solver;
int mgn_rollout(mgn_handle* h, mgn_rollout_desc* d);

/* ---- rollout with the errors reduced on the device: what _validation_step (reference src/strategies.jl:111-134, every strategy's
 * validation_step, run over every validation trajectory at every checkpoint of train_mgn!, src/MeshGraphNets.jl:404-467) and
 * eval_network! (:609-635) take from a rollout.  d is read exactly as mgn_rollout reads it (Euler, adaptive or fixed-step Tsit5, both time types,
 * both inflow rules, the in-place inflow overwrite; the same launches in the same order), d->n_accept / n_reject / n_rhs are filled, and
 * d->out MAY BE NULL: then no [n_saves][N][O] buffer is held on the device and nothing of that size is downloaded.  With d->out given
 * the predicted saves are bit-identical to mgn_rollout's.  As each save i is produced it is compared with gt[i]:
 *   mse_save[i][o] = mean over the N nodes of (x_i - gt_i)^2            eval_network!'s `error` (mean(...; dims = 2), :615-619)
 *   mse_time[n][o] = mean over the n_saves saves of (x_i - gt_i)^2      _validation_step's `error` (mean(...; dims = 3), :131)
 *   val_loss       = mean of mse_time over sel                         _validation_step's `mean(error[mask])`
 * sel holds LINEAR indices into the row-major [N][O] array mse_time (the bytes of Julia's O x N `error`): the reference indexes that
 * matrix with the vector of node indices `mask` (src/MeshGraphNets.jl:415-417), which is linear indexing -- element sel[i] -
 * sel_index_base, not "all components of node sel[i]" -- so sel = mask with sel_index_base = 1 reproduces validation_step exactly.  A
 * caller who wants whole nodes passes the expanded indices node * O + o.  Duplicates count as often as they are listed; indices refer
 * to the caller's node order.  n_sel == 0: the mean over all N * O elements.
 * gt: host or device pointer (hipMemcpyDefault), caller's order.  If gt is the same pointer as d->inflow_data (ground truth IS the
 * inflow data in validation) and d->n_frames >= d->n_saves, the frames uploaded for the right-hand side are compared against and gt is
 * not uploaded again; the results are the same bits either way.  mse_time: host or device pointer.
 * Differences and squares are formed in double from the fp32 values and accumulated in double on the device; mse_time is rounded to
 * float once, mse_save and val_loss come from the double sums.  Every reduction has a fixed order that depends on N, O and n_saves
 * alone (no floating-point atomics): bitwise repeatable.  One synchronisation, at the end.
 * Refusals: everything mgn_rollout refuses; MGN_E_ARG for a NULL e or gt, n_gt < n_saves, n_sel < 0, n_sel > 0 without sel, a
 * sel_index_base other than 0 or 1, a sel entry outside [0, N * O); MGN_E_UNSUPPORTED on a partitioned handle (nranks != 1: call
 * mgn_rollout and reduce on the host, or drive the partitions through a group: mgn_group_rollout_eval reduces on the ranks).  The
 * handle stays usable after any of them.                                                                                           */
typedef struct mgn_rollout_eval_desc {
    const float* gt;        /* [n_gt][N][O], host or device, caller's node order; may be the same pointer as d->inflow_data         */
    int32_t n_gt;           /* >= d->n_saves; save i is compared with gt[i]                                                          */
    double* mse_save;       /* out, host [n_saves][O], or NULL                                                                       */
    float* mse_time;        /* out, host or device [N][O], caller's node order, or NULL                                              */
    const int32_t* sel;     /* host [n_sel] linear indices into [N][O], or NULL                                                      */
    int64_t n_sel;
    int32_t sel_index_base; /* 0 or 1                                                                                                */
    double val_loss;        /* out                                                                                                   */
} mgn_rollout_eval_desc;
int mgn_rollout_eval(mgn_handle* h, mgn_rollout_desc* d, mgn_rollout_eval_desc* e);

/* ---- explicit Runge-Kutta by tableau: the reference types every solver argument as OrdinaryDiffEqAlgorithm (`solver_valid`, the
 * `solver` of eval_network, src/MeshGraphNets.jl:53), so RK4(), BS3(), DP5(), Heun() or Midpoint() may arrive.  A Butcher tableau is
 * DATA here: a flat array of MGN_ERK_TABLEAU_DOUBLES doubles, filled by mgn_erk_named or by the caller, checked by mgn_erk_check, and
 * handed to the *_erk entry points below, which drive the same resident right-hand side, saves, error reduction, controller and
 * partitions as mgn_rollout.  Up to MGN_ERK_MAX_STAGES stages; host only, no handle.
 *   tab[0] stages s (1..7)   tab[1] order p (>= 1)   tab[2] fsal (0/1)   tab[3] embedded (0/1)
 *   tab[4] beta1  tab[5] beta2  (PI controller; 0, 0 = the defaults 7/(10 p), 2/(5 p))
 *   tab[6 + 7 i + j] = A[i][j], 0-based, used for j < i      tab[55 + i] = b[i]
 *   tab[62 + i] = c[i]      tab[69 + i] = btilde[i] = b[i] - bhat[i]  (embedded only)
 * mgn_erk_check answers MGN_E_ARG for: a NULL tab; stages outside 1..7; a non-integral header entry (stages, order, fsal, embedded);
 * anything non-finite; a non-zero A[i][j] with j >= i inside the s x s block; |sum b - 1| > 1e-10; order < 1; embedded with
 * |sum btilde| > 1e-10; fsal without b[s-1] == 0, c[s-1] == 1 and A[s-1][j] == b[j] for all j (compared exactly); a negative beta.
 * mgn_erk_named fills tab (zeros elsewhere) with a named method: Euler; Heun (OrdinaryDiffEq's explicit trapezoid), Midpoint, Ralston
 * (p = 2); RK4 (the classical one); BS3 (Bogacki-Shampine 3(2), FSAL, embedded); DP5 (Dormand-Prince 5(4), FSAL, embedded, beta1 = 0.17,
 * beta2 = 0.04); Tsit5 (the tableau MGN_SOLVER_TSIT5 drives: FSAL, embedded, the default betas 7/50 and 2/25).  MGN_E_ARG for a name
 * outside the enum or a NULL tab.                                                                                                    */
#define MGN_ERK_MAX_STAGES 7
#define MGN_ERK_TABLEAU_DOUBLES 76
typedef enum mgn_erk_name { MGN_ERK_EULER = 0, MGN_ERK_HEUN = 1, MGN_ERK_MIDPOINT = 2, MGN_ERK_RALSTON = 3,
                            MGN_ERK_RK4 = 4, MGN_ERK_BS3 = 5, MGN_ERK_DP5 = 6, MGN_ERK_TSIT5 = 7 } mgn_erk_name;
int mgn_erk_named(int32_t name, double* tab /* [MGN_ERK_TABLEAU_DOUBLES] */);
int mgn_erk_check(const double* tab);   /* MGN_OK or MGN_E_ARG */

/* mgn_rollout / mgn_rollout_eval with the method given by a tableau.  d is read as mgn_rollout reads it -- both time types, both inflow
 * rules, the in-place inflow overwrite, d->out optional in the eval form, n_accept / n_reject / n_rhs filled -- except d->solver, which
 * is ignored.  mgn_erk_check runs before anything else (a bad tableau is MGN_E_ARG on every handle, a host-only one included).
 *   Stage input y_i = x_n + h sum_{j<i} A[i][j] k_j: coefficients rounded to float once, terms whose coefficient is exactly 0 left out,
 *   the rest in ascending j through mgn_rollout's fmaf chain.  Stage 1 sees t_n; the FSAL stage (stage s of an FSAL tableau) is evaluated
 *   on x_{n+1} and sees t_{n+1}; every other stage sees t_n + c_i h, each operation rounded to the time type.  Each right-hand side
 *   overwrites the inflow rows of the array it is evaluated on, in place: with FSAL a saved x_{n+1} carries the rows of frame(t_{n+1});
 *   without, the save is x_{n+1} as the update left it and stage 1 of the next step overwrites it (what MGN_SOLVER_EULER does).
 *   FSAL: the last stage of an accepted step is k_1 of the next, n_rhs = 1 + (s - 1)(n_accept + n_reject).  Otherwise k_1 is evaluated
 *   once per state that starts a step (a retrial reuses it), n_rhs = n_accept + (s - 1)(n_accept + n_reject).
 * adaptive = 0: solve(prob, alg; adaptive = false, dt, saveat = saves).  dt > 0, else MGN_E_ARG.  K = round((t1 - t0) / dt) steps,
 *   t <- t + dt in the time type (the last step snaps onto t1), every save must be reached.  A general tableau has no dense output here:
 *   saves_dt / dt must be an integer >= 1 to within 1e-6 relative, else MGN_E_ARG (Tsit5 with other steps is MGN_SOLVER_TSIT5_FIXED).
 *   abstol / reltol are ignored; no error norm: no D2H copy per step and, on partitions, no reduction per step.
 * adaptive = 1: solve(prob, alg; saveat = saves, tstops = saves): MGN_SOLVER_TSIT5's loop -- stops, padding, the rank-reduced error norm,
 *   the iteration guard -- with the tableau's stages and btilde, the PI controller's beta1 / beta2 from the tableau and the exponent 1/p
 *   in the Hairer-Wanner start (d->dt == 0).  Needs an embedded pair, else MGN_E_UNSUPPORTED, and tolerances > 0, else MGN_E_ARG.
 *   With mgn_erk_named's Tsit5 tableau the result is MGN_SOLVER_TSIT5's, bit for bit, counters included.
 * Any other value of adaptive is MGN_E_ARG.  The group forms serve partitions as mgn_group_rollout / mgn_group_rollout_eval do.
 * d->dt == 0 with adaptive = 1 costs one more right-hand side than the formulas above (the Hairer-Wanner start's probe), as it does
 * for MGN_SOLVER_TSIT5.
 * Not built: dense output for a general tableau; adaptive training, mgn_shooting_grad and a group form of mgn_solver_grad_erk with a
 * tableau; implicit or stabilised methods; more than seven stages.                                                                     */
int mgn_rollout_erk(mgn_handle* h, mgn_rollout_desc* d, const double* tab, int32_t adaptive);
int mgn_rollout_eval_erk(mgn_handle* h, mgn_rollout_desc* d, mgn_rollout_eval_desc* e, const double* tab, int32_t adaptive);

/* ---- solver-based training: the loss and d loss / d ps of one fixed-step Euler solve of ode_func_train (reference src/solve.jl:101-117,
 * strategies.jl:175-196) -- what train_step(::SolverTraining) (strategies.jl:257-292) and one window of train_step(::MultipleShooting)
 * (:312-383) differentiate, with no host work per step and one synchronisation at the end.
 * d is read as mgn_rollout reads it (same fields, time type, inflow_rule, Euler time loop and save rule), with two differences: only
 * solver 0 (Euler; Tsit5 answers MGN_E_UNSUPPORTED: it is mgn_solver_grad_tsit5), and the inflow overwrite takes ode_func_train's form -- the rows go into a COPY the
 * right-hand side is evaluated on, the state itself is never overwritten.  Every save point must be reached (else MGN_E_ARG).
 *   loss = mean over (save s, node n, component o) of (loss_scale[o] (gt[s][n][o] - x_s[n][o]))^2 vm[n]  +  cont_weight sum |x_end - cont_target|
 * with the mean over n_saves * N * O, vm = d->val_mask (NULL: 1), loss_scale [O] (NULL: 1; the scale of the field normaliser, whose shift
 * cancels), cont_target [N][O] (NULL: no continuity term; MultipleShooting's, strategies.jl:376-378, subgradient 0 at 0).
 * gt [n_saves][N][O].  grads [n_grads = mgn_param_count] receives the EXACT gradient of that loss of the computed Euler solution (the
 * discrete adjoint, what ReverseDiffAdjoint / ZygoteAdjoint give -- not InterpolatingAdjoint's continuous approximation); d->out, if not
 * NULL, the predicted saves; d->n_accept, d->n_rhs are filled.  gt, cont_target and grads may be host or device pointers (hipMemcpyDefault);
 * the others follow mgn_rollout.  fp32, one partition, one edge set, hidden_layers 1 .. 4, both ln_mode and ln_dims values,
 * Fn, Fe, O <= L (MGN_E_UNSUPPORTED above: mgn_config, "Widths"; the same for mgn_solver_grad_tsit5, _erk and mgn_shooting_grad).  Memory: the
 * (K + 1) N O floats of the states before every step (4.8 GB for 1 M nodes over 600 steps); MGN_E_OOM when they do not fit.
 * Bitwise repeatable (reductions in a fixed order).                                                                                  */
int mgn_solver_grad(mgn_handle* h, mgn_rollout_desc* d, const float* gt /* [n_saves][N][O] */, const float* loss_scale /* [O] or NULL */,
                    const float* cont_target /* [N][O] or NULL */, float cont_weight, float* grads, size_t n_grads, float* loss);

/* ---- solver-based training with Tsit5 (the package's default solver, src/MeshGraphNets.jl:53): mgn_solver_grad's loss (same gt,
 * loss_scale, cont_target, cont_weight, grads, loss; same host-or-device rules and refusals) of one window of ode_func_train solved by
 * the Tsitouras 5(4) pair, and its gradient.  d is read as mgn_solver_grad reads it, with d->solver = 1 (else MGN_E_ARG); d->out receives
 * the predicted saves, d->n_accept / n_reject / n_rhs are filled.  For accepted step n from t_n with size h_n, i = 1 .. 6 (A[i][j] 1-based,
 * b = A[7]):
 *   y_{n,i} = x_n + h_n sum_{j<i} A[i][j] k_{n,j};   z_{n,i} = y_{n,i} with the inflow rows of frame(t_n + c_i h_n) (a COPY);
 *   k_{n,i} = f(z_{n,i});   x_{n+1} = x_n + h_n sum_i A[7][i] k_{n,i}   (k_7 = f(z_{n+1,1}), FSAL, feeds the error estimate only)
 * The gradient is the DISCRETE ADJOINT OF THE COMPUTED SOLUTION WITH THE ACCEPTED STEP SEQUENCE HELD FIXED: step sizes and accept / reject
 * decisions are constants (the error norm carries no derivative), rejected trials contribute nothing -- the usual convention for
 * differentiating through an adaptive integrator; it is not InterpolatingAdjoint's continuous adjoint.  Reverse, from lam = dL/dx_{n+1}:
 *   for i = 6 .. 1:  kbar_i = h_n (A[7][i] lam + sum_{j>i} A[j][i] ybar_j);  zbar_i, g_i = VJP of f at z_{n,i};  ybar_i = zbar_i with
 *   the inflow rows zeroed;  gs += g_i.        dL/dx_n = lam + sum_i ybar_i + the save / continuity terms at x_n.
 * Step modes (o->adaptive, a set of flags: MGN_TSIT5_ADAPTIVE | MGN_TSIT5_DENSE_SAVES; any other bit is MGN_E_ARG):
 *   1: solve(prob, Tsit5(); saveat = saves, tstops = saves) -- mgn_rollout's Tsit5 unchanged: first step d->dt (0: Hairer-Wanner), PI
 *      controller, d->abstol / d->reltol, stops, stage times.  The error norm is taken on the states, which are not overwritten: with an
 *      inflow mask the steps can differ from mgn_rollout's, which overwrites in place.  The stage-7 input is z_{n+1,1} and sees t_{n+1}.
 *      More than 100 000 accepted steps (OrdinaryDiffEq's maxiters) or a NaN error estimate: MGN_E_STATE.
 *   0: solve(...; adaptive = false, dt): steps of d->dt on mgn_solver_grad's Euler time grid and save rule (last step snapped onto t1;
 *      every save must be reached, else MGN_E_ARG).  Its loss is a smooth function of the parameters.
 *   In modes 0 and 1 every save is stepped onto (tstops = saves) and d->out is bit-identical to mgn_rollout's solution.
 *   3: solve(prob, Tsit5(); saveat = saves), NO tstops -- what the reference's MultipleShooting solves every window with
 *      (src/strategies.jl:343-355).  Controller, first step and stage times as mode 1; the only stop is t1.
 *   2: solve(...; adaptive = false, dt, saveat = saves): t <- t + dt in the solver's time type with h = dt; a step whose end lies within
 *      1e-5 saves_dt of t1 snaps onto t1, one that would pass t1 is cut to h = t1 - t.  dt need not divide saves_dt.
 *   Dense saves (modes 2 and 3): after accepted step n (t_n to t_{n+1}, size h_n) every pending save time t_s <= t_{n+1} is taken.  One
 *   with |t_s - t_{n+1}| <= 1e-9 |t_{n+1}| + 1e-12 is x_{n+1} itself, a loss term of that state as in modes 0 and 1.  Any other is
 *   Tsit5's dense output xhat_s = x_n + h_n sum_{i=1..7} b_i(theta_s) k_{n,i}, theta_s = (t_s - t_n) / h_n in double (at most 1), b from
 *   mgn_tsit5_interp_weights rounded to float once, k_{n,7} = f(z_{n+1,1}).  The save at t0 is x0; saves the solve stops short of are
 *   the final state.  The adjoint holds h_n and theta_s fixed: with ghat_s = dL/dxhat_s and S_n the interpolated saves of step n,
 *     lam_n += sum_{S_n} ghat_s;  kbar_{n,i} += h_n sum_{S_n} b_i(theta_s) ghat_s (i = 1 .. 6);  kbar_{n+1,1} += h_n sum_{S_n} b_7(theta_s) ghat_s
 *   (k_{n,7} is the evaluation k_{n+1,1}; for the last step one extra VJP at z_{K,1}, its output with the inflow rows zeroed added to lam_K).
 *   step_t / step_h record the h every step used.  A save time an ulp short of t1 is interpolated at theta just below 1: pass the t1 the
 *   save grid gives (t0 + (n_saves - 1) saves_dt in the solver's time type) to have the last save be the final state.
 * Memory: the six stage inputs z_{n,1..6} of every accepted step, 6 N O floats per step, in chunks kept on the handle and grown as steps
 * are accepted, and with dense saves 7 N O floats of sums; allocation failure or more than o->max_store_bytes (0: no limit) of the two
 * together is MGN_E_OOM, and the handle stays usable.
 * Through mgn_group_solver_grad_tsit5 the memory and max_store_bytes are PER RANK (6 n_own O floats per step on each rank, 7 n_own O of sums).
 * Bitwise repeatable.                                                                                                             */
#define MGN_TSIT5_ADAPTIVE 1     /* PI-controlled steps (else fixed steps of d->dt)                                                  */
#define MGN_TSIT5_DENSE_SAVES 2  /* no stop but t1; saves between steps come from Tsit5's dense output (else tstops = saves)          */
/* Tsit5's dense-output weights b_1 .. b_7 at theta in [0, 1] (the free 4th-order interpolant of Tsitouras 2011, as OrdinaryDiffEq.jl's):
 * x(t_n + theta h) = x_n + h sum_i b[i - 1] k_i.  Host only, no handle.  MGN_E_ARG for a theta outside [0, 1] (NaN included) or b NULL. */
int mgn_tsit5_interp_weights(double theta, double b[7]);
typedef struct mgn_solver_grad_opts {
    int32_t adaptive;          /* step mode: MGN_TSIT5_ADAPTIVE | MGN_TSIT5_DENSE_SAVES (0 .. 3, see above)                        */
    int32_t step_cap;          /* capacity of step_t / step_h (0: no record)                                                       */
    double* step_t;            /* out [step_cap] or NULL: start time of every accepted step, in the solver's time type               */
    double* step_h;            /* out [step_cap] or NULL: the h the stage combinations of that step used                             */
    size_t max_store_bytes;    /* 0: bounded by device memory only; else the stored stage inputs (+ dense sums) may not exceed it    */
    int32_t n_steps;           /* out: accepted steps (only the first step_cap are recorded)                                         */
    size_t stored_bytes;       /* out: bytes the stored stage inputs took (+ the 7 N O floats of sums with dense saves)              */
} mgn_solver_grad_opts;
int mgn_solver_grad_tsit5(mgn_handle* h, mgn_rollout_desc* d, mgn_solver_grad_opts* o, const float* gt /* [n_saves][N][O] */,
                          const float* loss_scale /* [O] or NULL */, const float* cont_target /* [N][O] or NULL */, float cont_weight,
                          float* grads, size_t n_grads, float* loss);

/* ---- MultipleShooting as one batch: the summed loss and gradient of the W windows of train_step(::MultipleShooting) (reference
 * src/strategies.jl:312-383).  The result is the sum of the W single-window calls train_step_multiple_shooting makes one by one: window w
 * is mgn_solver_grad (d->solver 0) or mgn_solver_grad_tsit5 with adaptive = 0 (d->solver 1) with x0 = gt[first[w]], t0 = t0[w], t1 = t1[w],
 * n_saves = last[w] - first[w] + 1, gt = gt[first[w] .. last[w]], cont_target = gt[first[w + 1]] and cont_weight for w < W - 1 (no
 * continuity term for the last window), everything else (dt, saves_dt, time_f64, inflow_rule, node_type_onehot, ef_raw, val_mask,
 * inflow_mask, inflow_data / n_frames) from d and loss_scale as given.  Inflow frames are chosen by absolute time, so each window reads its
 * own.  d->x0, d->t0, d->t1 and d->n_saves are ignored.  *loss: the summed loss; grads: the summed discrete-adjoint gradient; d->out, if not
 * NULL, the predicted saves [sum_w n_saves_w][N][O] in window order; d->n_accept / d->n_rhs: the totals.
 * Windows are independent (each starts from ground truth; the continuity term couples window w only to gt), so windows whose step plans
 * are identical (same step count, save steps and step size) are solved together as one block-diagonal graph of B copies of the mesh, on a
 * companion engine the handle keeps (released by mgn_set_graph / mgn_set_graph_local / mgn_destroy).  A pass of one window runs on the
 * handle itself.  With ln_dims = MGN_LN_ALL the statistics of a LayerNorm would couple the copies: every pass holds one window there.
 * Restrictions, pointer kinds (gt and grads: host or device) and refusals as mgn_solver_grad; Tsit5 with adaptive != 0 is MGN_E_UNSUPPORTED,
 * W < 1 or a window outside gt MGN_E_ARG.  Bitwise repeatable; one synchronisation at the end.                                         */
typedef struct mgn_shooting_desc {
    int32_t n_windows;            /* W >= 1                                                                                          */
    const int32_t* first;         /* [W] 0-based index into gt of window w's first save: u0 = gt[first[w]]                           */
    const int32_t* last;          /* [W] inclusive; last[w] > first[w]; n_saves_w = last[w] - first[w] + 1                           */
    const double* t0;             /* [W] the window's tspan in the solver's time type (Julia: tsteps[first(rg)])                     */
    const double* t1;             /* [W]                                                                                             */
    int32_t n_gt;                 /* frames in gt                                                                                    */
    int32_t adaptive;             /* solver 1 (Tsit5): must be 0 (fixed steps of d->dt); adaptive is refused                         */
    int32_t max_windows_per_pass; /* 0: no cap other than max_batch_nodes                                                            */
    int64_t max_batch_nodes;      /* 0: 1 << 20; a pass holds at most max(1, floor(this / N)) windows                                */
    int32_t n_groups, n_passes;   /* out                                                                                             */
} mgn_shooting_desc;
/* ---- mgn_solver_grad_tsit5's loss and gradient for an explicit Runge-Kutta tableau (mgn_erk_named / mgn_erk_check above): the `solver` of
 * SolverTraining and MultipleShooting is any OrdinaryDiffEqAlgorithm (reference src/strategies.jl:242,316).  Arguments, host-or-device
 * rules and refusals are mgn_solver_grad_tsit5's; d->solver is not read; mgn_erk_check runs before anything else.  Fixed steps only:
 * o->adaptive must be 0, MGN_E_UNSUPPORTED otherwise.  The grid and saves are those of mgn_rollout_erk with adaptive = 0 (dt > 0,
 * saves_dt / dt an integer >= 1, every save reached), the inflow overwrite takes the training form (copies; the state is never
 * overwritten).  With s' = s - fsal active stages (s' <= 6, else MGN_E_UNSUPPORTED):
 *   forward   z_{n,i} = x_n + h sum_{j<i} A[i][j] k_{n,j} with the inflow rows of frame(t_{n,i}), in a copy;  k_{n,i} = f(z_{n,i});
 *             x_{n+1} = x_n + h sum_i b_i k_{n,i}
 *   reverse   from lam = dL/dx_{n+1}, for i = s' .. 1:  kbar_i = h (b_i lam + sum_{j>i} A[j][i] ybar_j);  (zbar_i, g_i) = VJP at z_{n,i};
 *             ybar_i = zbar_i with the inflow rows zeroed;  gs += g_i;  then dL/dx_n = lam + sum_i ybar_i + the save / continuity terms
 * -- the exact gradient of the computed solution.  Stored: s' N O floats per step in the chunks mgn_solver_grad_tsit5 uses;
 * max_store_bytes, stored_bytes, step_t, step_h and n_steps behave as there.  d->out is bit-identical to mgn_rollout_erk's solution
 * where there is no inflow mask.  With mgn_erk_named's Tsit5 tableau: mgn_solver_grad_tsit5's bits in step mode 0.                       */
int mgn_solver_grad_erk(mgn_handle* h, mgn_rollout_desc* d, const double* tab, mgn_solver_grad_opts* o, const float* gt,
                        const float* loss_scale, const float* cont_target, float cont_weight, float* grads, size_t n_grads, float* loss);
int mgn_shooting_grad(mgn_handle* h, mgn_rollout_desc* d, mgn_shooting_desc* s, const float* gt /* [n_gt][N][O] */,
                      const float* loss_scale /* [O] or NULL */, float cont_weight, float* grads, size_t n_grads, float* loss);

/* ---- training step -------------------------------------------------------
 * GraphNetCore.step!(mgn, graph, target, mask, mse_reduce) as called at reference src/strategies.jl:418-422 and
 * consumed at src/MeshGraphNets.jl:370-378:  out = model(graph);  loss = mean(mse_reduce(target, out)[mask]) with
 * mse_reduce = sum of squared differences over the O rows per node;  gs = d loss / d ps.
 *   nf [N][Fn], ef [E][Fe]: the FeatureGraph (already normalised, as build_graph hands it over, src/graph.jl:75-97)
 *   target [N][O];  mask [nmask]: node indices (Int32, 1-based at the Julia boundary: mask_index_base = 1,
 *   src/MeshGraphNets.jl:352);  grads [n_grads = mgn_param_count]: packed order of mgn_set_params, so that
 *   Optimisers.update(opt_state, ps, gs) keeps working on the Julia side;  *loss: the scalar.
 * fp32; both ln_mode values and both ln_dims values; hidden_layers 1 .. 4; with two edge sets the second set's
 * features are the ones installed by mgn_set_edge_features (as in mgn_forward).
 * Restrictions on the widths: Fn, Fe, Fe2, O <= L for this and every other training entry point (mgn_step_datapoint, mgn_step_datapoints
 * and the resident trajectory's calls, mgn_ode_vjp, mgn_forward_vjp, mgn_solver_grad*, mgn_shooting_grad, the mgn_group_* forms): a wider
 * configuration is answered with MGN_E_UNSUPPORTED, the message naming the width and L, before the device check and before any
 * allocation, launch or collective (mgn_config, "Widths").  Inference on MGN_LN_ROWS has no such bound.
 * Partitioned mesh (nranks > 1, after mgn_comm_init; one edge set): every rank calls with the GLOBAL nf [N][Fn], ef [E][Fe],
 * target [N][O] and the mask of the whole mesh (global node ids) and returns the COMPLETE gradient and the loss of the whole mesh,
 * the same bits on every rank.  Each rank computes on the rows it owns plus its halo rows and takes the mask entries it owns (the
 * divisor is nmask; a rank that owns none still takes part in every exchange).  Forward: the owned boundary rows of v go to the
 * peers that list them as halo after the node encoder and after every node MLP but the last (mps exchanges of L floats per row).
 * Reverse: the halo rows' gradients w.r.t. v_k go back over the same lists and the owner adds them to its own term before it
 * unwinds node MLP k - 1 -- own term, then peers in ascending rank, then list order; no floating-point atomics.  Finish: the
 * ranks' gradients and loss numerators are gathered and added in ascending rank order in double by the same kernel on every rank;
 * the call blocks once, there.  It runs eagerly on the handle's stream (no hipGraph replay, no second stream); stored / recomputed
 * steps are decided per rank for its own arena.  Refusals: MGN_E_STATE naming mgn_comm_init without a communicator,
 * MGN_E_UNSUPPORTED with two edge sets, MGN_E_ARG for a wrong n_grads -- all before the first collective, so no rank is left
 * waiting.  The other training entry points (mgn_ode_vjp, mgn_forward_vjp, mgn_solver_grad, mgn_solver_grad_tsit5,
 * mgn_shooting_grad) drive one partition on rank handles: MGN_E_STATE on a partitioned handle.  Their partitioned forms are reached
 * through the group: see mgn_group_ode_vjp, mgn_group_forward_vjp, mgn_group_solver_grad and mgn_group_solver_grad_tsit5.
 * Memory: a large mesh stores the activations of as
 * many processor steps as the device's free memory (hipMemGetInfo) minus MGN_TRAIN_RESERVE_GB (16) holds and recomputes the others
 * in the reverse pass -- the first handle on a device takes the stored steps, a later one recomputes; a refused allocation is retried
 * with fewer stored steps, MGN_E_OOM only when the arena without any does not fit (M-1M: 61 GB + 10.7 GB per stored step).  Deterministic: gradients are reduced in a fixed order; the only atomic
 * (the scalar loss / per-node seed when `mask` lists a node twice) adds identical terms, so the order does not matter.
 * nf, ef, target and grads may be HOST or DEVICE pointers (copied with hipMemcpyDefault on the handle's stream): with
 * device arrays -- the reference keeps graph, ps and gs on the GPU, src/MeshGraphNets.jl:255-263 -- the optimiser update
 * runs where the gradients are and no 4 x param_count bytes cross PCIe per step.  mask is read on the host.        */
int mgn_step(mgn_handle* h, const float* nf, const float* ef, const float* target, const int32_t* mask, int64_t nmask,
             int32_t mask_index_base, float* grads, size_t n_grads, float* loss);

/* ---- derivative training on a device-resident trajectory -----------------------------------------------------------------
 * The loop `for datapoint in 1:delta` of the reference's default strategy (DerivativeTraining, src/MeshGraphNets.jl:364-378:
 * init_train_step -> step! -> Optimisers.update) without host work per datapoint.  The reference puts the fields, their `target|`
 * copies and the noise on the device once per trajectory (add_targets! and preprocess!, src/dataset.jl:461-509) and forms
 * o_norm((next - cur) / dt) and build_graph there once per datapoint (init_train_step of the derivative strategies,
 * src/strategies.jl:395-416); these entry points do the same.  Optimisers.update and the order in which datapoints are visited
 * stay with the caller.  fp32 (MGN_E_STATE otherwise); every array may be a host or a device pointer unless noted.  One partition,
 * or a partitioned mesh after mgn_comm_init: "On a partitioned mesh" below.
 *
 * mgn_train_set_trajectory, once per trajectory and after the graph is complete (mgn_set_graph, and mgn_set_edge_set where there
 * is a second set): frames [T][N][O] holds frame t = data[field][:, :, t] of the target fields, concatenated in output order, in
 * the caller's node order; T >= 2, and the last frame is only ever a target (what add_targets! makes of a trajectory), so the
 * datapoints are 0 .. T - 2.  The time step of datapoint t is times[t + 1] - times[t] (fp32), or dt when times == NULL.
 * node_type_onehot [N][Fn - O]: the one-hot columns that follow the O state columns, as in mgn_ode_step; ef_raw [E][Fe] in the
 * caller's edge order.  All three are brought into the engine's order here, once: no gather per step remains.  A new graph and
 * mgn_destroy drop the trajectory and the noise settings; mgn_set_params (a training loop calls it before every step) and
 * mgn_set_norms do not.  The call blocks until the arrays have left the caller's memory.
 *
 * mgn_train_set_noise (preprocess!, src/dataset.jl:496-509): the input state of datapoint t is
 *     cur_t[n][o] = frames[t][n][o] + stddev[o] * z(seed, t, n, o)     on nodes with noisy[n] != 0 (noisy == NULL: every node),
 * frames[t] exactly on the others, and everywhere when stddev == NULL.  z is the engine's N(0,1) generator (splitmix64 of the
 * key, Box-Muller; the one mgn_latents_randn uses) on the trajectory as a [T N][O] array: key (seed, row t N + n, column o) with n
 * the CALLER's node id, so the noise does not depend on the engine's numbering.  The product and the sum are rounded one by one.
 * The next state frames[t + 1] carries no noise: the reference adds it to data[field], not to data["target|field"].  noisy [N] is
 * read on the host.  The settings hold for later trajectories on the same graph.
 *
 * What a datapoint is made of, all in fp32 with IEEE subtraction and division, one rounding each (no contraction, no fast divide):
 *     d      = (frames[t + 1] - cur_t) / delta                    the raw target
 *     target = (d - out_shift) / out_scale                        the forward of the normaliser whose inverse mgn_set_norms holds
 *     nf     = [cur_t ; onehot] * node_scale + node_shift         ef = ef_raw * edge_scale + edge_shift
 * nf and ef are zero-padded to L and use the very expression the right-hand side's inputs are staged with, so they carry the bits
 * mgn_ode_vjp computes with for the same raw inputs.  A map mgn_set_norms left out is the identity.
 *
 * mgn_step_datapoint is mgn_step on these arrays: mask, mask_index_base, grads, n_grads and loss as there (mask on the host, grads a
 * host or device pointer), its argument checks, one or two edge sets (the second set's features installed by
 * mgn_set_edge_features), hidden_layers, ln_mode, ln_dims, the arena plan and the hipGraph replay of small meshes all unchanged.
 * The normalised edge rows are kept and rebuilt only when the trajectory or the norms change.
 *
 * Online normalisers (GraphNetCore NormaliserOnline): mgn_train_online_norms switches a group -- the node STATE columns, the edge
 * features, the output -- to online and zeroes its totals (sum, sum of squares, count, calls); a group left off keeps what
 * mgn_set_norms gave it, and the one-hot columns are never online (the reference gives node_type an offline min-max normaliser).
 * The state outlives graphs and trajectories, as the normalisers of the reference's model do.  With accumulate != 0 every online
 * group with calls < max_accumulations first adds this datapoint's raw rows -- cur_t (N rows), ef_raw (E rows), d (N rows), in the
 * caller's order -- to double totals that live on the device: mgn_feature_stats' reduction in mgn_feature_stats' order, so the
 * totals are bitwise repeatable and equal the running sum of that entry point's results on the exported raw arrays (the sums of
 * ef_raw are formed once per trajectory and added per call).  One small kernel then rewrites the group's entries of the norms:
 * mean and std = sqrt(max(sumsq / c - mean^2, 0)) in double, rounded to float, std = max(std, std_epsilon); scale = 1.0f / std,
 * shift = -mean * scale; the output group stores std, mean.  The datapoint is normalised with the updated maps (the reference's
 * normaliser call accumulates, then normalises).  No copy to the host and no synchronisation are added; count and calls are host
 * numbers.  With accumulate == 0 the maps are used as they stand (a later mgn_set_norms overwrites an online group's entries, too,
 * until that group's next accumulating step).  Every later entry point on the handle computes with the
 * rewritten norms; the resident right-hand side of mgn_set_static is invalidated as mgn_set_norms invalidates it.
 * mgn_train_norm_state reads (write = 0) or restores (write = 1) a group's totals and count_and_calls = {count, calls}: the
 * checkpoint hook for save! / load.  Restored totals give the group's map at the next datapoint; sum and sum_squares are host
 * arrays of O, Fe, O doubles for groups 0, 1, 2.
 *
 * mgn_datapoint_export returns, in the caller's order, what the step consumes (normalised != 0: nf, ef, target as above, unpadded)
 * or the raw arrays (normalised == 0: [cur_t ; onehot], ef_raw and d).  Any output may be NULL.  It never accumulates.
 *
 * On a partitioned mesh (nranks > 1, after mgn_comm_init; one edge set, MGN_E_UNSUPPORTED with two) all six calls follow the
 * nranks > 1 contract of mgn_step: every rank is given the same arrays of the WHOLE mesh -- frames [T][N][O], node_type_onehot, ef_raw
 * [E][Fe], noisy [N], mask with the caller's node ids -- and the same arguments, and every rank gets the complete gradient and the loss,
 * the same bits on every rank.  A rank keeps on the device only the rows of the nodes it owns ([T][n_own][O], [n_own][Fn - O]) and of
 * its local edges, in the engine's order; the mesh's arrays pass through a staging buffer that does not grow with T (a whole number
 * of frames, at least one, at a time; the one-hot rows; the edge features).  The noise key is (seed, row t N + n, column o) with N and
 * n of the whole mesh: the noisy state of a node is the same bits for every number of ranks and every partition.
 * mgn_step_datapoint is mgn_step's partitioned path on the rank's rows (eager; forward and reverse halo exchange, rank-ordered finish);
 * every argument check precedes the first collective, so a refused call leaves no rank waiting.
 * Online normalisers: an accumulating step forms each rank's column sums and sums of squares of the cur_t and d rows it owns (block
 * partials added in block order), one allgather on the handle's stream brings the 4 O doubles of every rank to every rank, and the
 * ranks' parts are added to the totals in ASCENDING RANK ORDER in double.  Totals and maps are the same bits on every rank and
 * repeatable for a given partition; they agree with the single-partition totals up to double rounding, NOT bitwise (other partial
 * sums).  The sums of ef_raw are formed the same way once per trajectory (every edge lives on one rank).  count advances by N and E of
 * the whole mesh; whether a group accumulates depends only on arguments and counters all ranks share, so every rank -- one that owns
 * no edge, too -- joins every allgather.  No host copy and no synchronisation per step.  mgn_train_norm_state reads the totals of
 * the rank asked (all ranks hold the same); a restore must be given the same values on every rank.
 * mgn_datapoint_export on a partitioned handle takes HOST arrays of the whole mesh's shapes and writes the rows of the nodes this
 * rank owns and of its local edges (mgn_owned_nodes, mgn_local_edges), leaving the others untouched, as mgn_fwd_download does; it
 * joins no collective, so one rank may call it alone.
 *
 * Refusals, all before any launch, the handle stays usable: MGN_E_STATE without a graph, without a trajectory (step, export), on
 * a partitioned handle without a communicator (call mgn_comm_init) or with dtype != MGN_F32; MGN_E_ARG for T < 2, a datapoint outside [0, T - 2], Fn < O, a missing onehot
 * when Fn > O, a missing ef_raw with E > 0, a zero time step (checked on the host at upload), max_accumulations <= 0 or
 * std_epsilon <= 0, a group outside 0 .. 2, and what mgn_step refuses in its own arguments.                                   */
int mgn_train_set_trajectory(mgn_handle* h, const float* frames, int32_t T, const float* times, float dt,
                             const float* node_type_onehot, const float* ef_raw);
int mgn_train_set_noise(mgn_handle* h, const float* stddev, const uint8_t* noisy, uint64_t seed);
int mgn_train_online_norms(mgn_handle* h, int32_t node_on, int32_t edge_on, int32_t out_on, double max_accumulations, float std_epsilon);
int mgn_train_norm_state(mgn_handle* h, int32_t group, int32_t write, double* sum, double* sum_squares, double* count_and_calls);
int mgn_step_datapoint(mgn_handle* h, int32_t datapoint, int32_t accumulate, const int32_t* mask, int64_t nmask,
                       int32_t mask_index_base, float* grads, size_t n_grads, float* loss);
int mgn_datapoint_export(mgn_handle* h, int32_t datapoint, int32_t normalised, float* nf, float* ef, float* target);

/* A minibatch of datapoints of the resident trajectory in one training step: the reference's Args.batchsize ("Size per batch (not
 * implemented yet)", src/MeshGraphNets.jl:39,224) for the loop of src/MeshGraphNets.jl:364-378.  The result is step! on the
 * block-diagonal FeatureGraph of the B datapoints datapoints[0 .. B - 1] (host array; they may repeat and come in any order) with the
 * mask repeated per copy:
 *     loss_b = mgn_step_datapoint's loss on datapoint datapoints[b]: the mean of (out - target)^2 over the nmask x O masked entries
 *     loss   = (1 / B) sum_b loss_b            grads = the gradient of loss = the mean of the per-datapoint gradients, packed order
 *     losses[b] = loss_b                       (host [B]; NULL: not wanted)
 * mask (listed once), mask_index_base, grads (host or device pointer), n_grads and the argument checks are mgn_step_datapoint's.  The
 * noise of datapoint t is the same bits as in the single call: the key (seed, t N + caller's node id, o) does not know the batch.
 *
 * B == 1 is mgn_step_datapoint in every respect -- the same path, the same bits, two edge sets, ln_dims = MGN_LN_ALL and a partitioned
 * handle included -- with losses[0] = loss.  B > 1 runs on a companion engine holding B copies of the handle's graph in the handle's
 * own engine order (the one mgn_shooting_grad uses: two batch sizes are kept per handle, parameters are packed again only after
 * mgn_set_params changed them, a new graph and mgn_destroy drop them).  One launch assembles the B datapoints' nf and target into the
 * companion's arena; the trajectory's normalised edge rows are replicated there and rebuilt only when the trajectory, the norms, that
 * arena or B change; the masked loss keeps per-copy double partials in fixed slots and one fold yields every loss_b and their mean in
 * double, each rounded once.  Every later stage is mgn_step's on B N nodes and B E edges: its size regimes, arena plan and hipGraph
 * replay.  The handle's own training state is not touched: a later mgn_step_datapoint returns the bits it returned before.  Loss and
 * gradients are bitwise repeatable (where no mask entry repeats, as for mgn_step).
 *
 * Online normalisers (accumulate != 0) ACCUMULATE FIRST AND NORMALISE AFTERWARDS: the B datapoints' raw rows are added to the totals
 * one datapoint at a time in the order listed, each as one call -- count and calls advance per datapoint, a group stops adding once
 * calls reaches max_accumulations, each with mgn_step_datapoint's reduction in its order, so the totals after the call are bitwise
 * those that B accumulating mgn_step_datapoint calls leave -- and all B datapoints are then normalised with the resulting maps.  This
 * is NOT what B sequential calls compute: there datapoint b is normalised with the maps after b + 1 accumulations.  No host copy of
 * the norms and no synchronisation are added.
 *
 * Refusals, all before any launch, the handle stays usable.  MGN_E_ARG: NULL datapoints, mask, grads or loss; B < 1 or
 * B > MGN_DATAPOINT_BATCH_MAX; a datapoint outside [0, T - 2]; what mgn_step_datapoint refuses in its own arguments; B N or B E beyond
 * INT32_MAX.  MGN_E_STATE: no graph, no trajectory, dtype != MGN_F32, and for B > 1 a partitioned handle (nranks != 1: it drives one
 * partition).  MGN_E_UNSUPPORTED for B > 1 with two edge sets (the companion replicates one) and with ln_dims = MGN_LN_ALL (whole-array
 * statistics would span the batch, which is a different model).  MGN_E_OOM when the companion's arena does not fit.                  */
#define MGN_DATAPOINT_BATCH_MAX 64
int mgn_step_datapoints(mgn_handle* h, const int32_t* datapoints /* host [B] */, int32_t B, int32_t accumulate,
                        const int32_t* mask, int64_t nmask, int32_t mask_index_base,
                        float* grads, size_t n_grads, float* loss, float* losses /* host [B] or NULL */);

/* Vector-Jacobian product of the right-hand side f = mgn_ode_step (reference ode_step, src/solve.jl:188-219) for the
 * solver-based training strategies, where the adjoint of `solve` needs lambda^T df/dx and lambda^T df/dps per RHS
 * evaluation (ZygoteVJP inside the sensitivity algorithm, src/strategies.jl:175-196).  Inputs as mgn_ode_step (raw edge
 * features, frozen normalisers of mgn_set_norms); lambda [N][O]; outputs xbar [N][O], grads [n_grads] (packed order) and,
 * when dxdt != NULL, f(x) itself.  Every array argument may be a host or a device pointer (hipMemcpyDefault).       */
int mgn_ode_vjp(mgn_handle* h, const float* x, const float* node_type_onehot, const float* ef_raw, const float* val_mask,
                const float* lambda, float* dxdt, float* xbar, float* grads, size_t n_grads);

/* Pullback of mgn_forward, i.e. of the model call `output, st = mgn.model(graph, ps, mgn.st)` at reference src/solve.jl:200 -- what
 * Zygote needs from the shim when it differentiates ode_func_train / train_loss as written (src/strategies.jl:183-195: the
 * normalisers, build_graph, inverse_data and `.* val_mask` around the model stay Julia code and are differentiated there).
 * nf [N][Fn], ef [E][Fe]: the FeatureGraph as given to mgn_forward; ybar [N][O]: cotangent of the output; out [N][O] (may be NULL):
 * the output itself; nfbar [N][Fn] = ybar^T d out / d nf; grads [n_grads] = ybar^T d out / d ps (packed order).  The edge
 * features are constants of a trajectory (create_base_graph, src/graph.jl:25-55): no cotangent is formed for them.
 * Restrictions and pointer kinds as mgn_step.                                                                              */
int mgn_forward_vjp(mgn_handle* h, const float* nf, const float* ef, const float* ybar, float* out, float* nfbar, float* grads,
                    size_t n_grads);

/* ---- multi-GPU: the halo exchange lives INSIDE the library (SURVEY.md 8b "the engine owns ... RCCL communicators", 8e) ----
 * One process (or thread) per partition, one handle each (mgn_config.rank / nranks).  After mgn_comm_init every compute
 * entry point that documents it runs at nranks > 1 with no host involvement per step: mgn_processor_steps_dev drives, per
 * processor step, boundary projection -> pack -> sparse all-to-all-v (one grouped ncclSend / ncclRecv pair per neighbour, each
 * pair over its own xGMI link, on the communicator's stream) -> interior projection and interior edge tiles while the rows
 * are on the wire -> wait -> boundary edge tiles.  There is no precedent in the reference (single device,
 * src/MeshGraphNets.jl:255-263).
 * Training: mgn_step runs at nranks > 1 as well (see there): the same exchange forward, its reverse -- halo gradients back to
 * their owners, added in a fixed order -- in the backward pass, and a rank-ordered sum of the gradients at the end.  Without
 * overlap: every exchange is waited for where it is started.  The solver-based training entry points and the two VJPs refuse a
 * partitioned handle (MGN_E_STATE).
 *   transport MGN_COMM_RCCL: RCCL (needs one GPU per rank).
 *   transport MGN_COMM_HOST: POSIX shared memory on one node, rows staged through the host.  Lets several ranks share one GPU
 *     (tests), serves host-only handles, and is a fallback where RCCL cannot initialise; not the production wire.
 *   transport MGN_COMM_LOCAL: the ranks are THREADS of one process (what mgn_group is inside) and find each other through the id in a
 *     process-wide registry.  Device rows never leave the device: the receiving rank copies them out of the peer's send buffer with one
 *     kernel launch, ordered against the peer by HIP events alone -- no host staging, no stream synchronisation.  Ranks may share a
 *     device; peers on different devices are read in place where hipDeviceCanAccessPeer allows it and with hipMemcpyPeerAsync otherwise.
 *     Host-only handles exchange by memcpy.  An id made for one of HOST / LOCAL is refused by the other.
 * Bootstrap: ONE rank calls mgn_comm_unique_id and the host distributes the MGN_COMM_ID_BYTES bytes (MPI.bcast, a
 * torch.distributed store, a file), then every rank calls mgn_comm_init with them (collective: returns when all ranks have
 * joined).  mgn_comm_init_file does the distribution through a file on a shared filesystem: rank 0 writes it, the others wait
 * for it.  Errors of this group: MGN_E_RCCL.                                                                          */
#define MGN_COMM_ID_BYTES 128
typedef enum mgn_comm_transport { MGN_COMM_RCCL = 0, MGN_COMM_HOST = 1, MGN_COMM_LOCAL = 2 } mgn_comm_transport;
int mgn_comm_unique_id(void* id /* [MGN_COMM_ID_BYTES] */, int32_t transport);
int mgn_comm_init(mgn_handle* h, const void* id, size_t id_bytes, int32_t transport);
int mgn_comm_init_file(mgn_handle* h, const char* path, int32_t transport);
int mgn_comm_destroy(mgn_handle* h);            /* also done by mgn_destroy */
int mgn_comm_barrier(mgn_handle* h);            /* drains the handle's stream, then meets the peers */
/* x[n] (host) reduced over the ranks in place, op 0 = sum, 1 = max; the same bits on every rank (timing brackets, checksums) */
int mgn_comm_allreduce(mgn_handle* h, double* x, int32_t n, int32_t op);
/* One blocking halo exchange of the CURRENT P rows (what the staged driver does between steps); for hosts that drive the
 * fine-grained mgn_fwd_* / mgn_proc_* stages themselves. */
int mgn_halo_exchange(mgn_handle* h);
/* Any per-node rows on the HOST: own_rows [n_own][width] -> halo_rows [n_halo][width] (order of mgn_halo_nodes) through the
 * communicator; works on host-only handles (MGN_COMM_HOST transport).  E.g. positions of halo nodes. */
int mgn_halo_exchange_host(mgn_handle* h, const float* own_rows, float* halo_rows, int32_t width);

/* ---- one process, P partitions: a group drives every rank of an edge-cut partitioned mesh from ONE caller thread ---------------
 * What an MPI-style program does with one process, one handle and mgn_comm_init per rank, for callers that are one process holding
 * one model (the reference's train_network / eval_network, src/MeshGraphNets.jl:255-263).  mgn_group_create starts one worker thread
 * per rank (nranks of them, nothing is sized by the machine); worker k selects devices[k] once, owns an ordinary handle made by
 * mgn_create with rank = k, nranks and device = devices[k] (cfg->rank, cfg->nranks and cfg->device are ignored; ordinals may repeat:
 * ranks may share a GPU), and the ranks are joined by one MGN_COMM_LOCAL communicator.  devices[k] = MGN_DEVICE_NONE for every k gives
 * a host-only group: mgn_group_set_graph and the introspection of its rank handles work, compute answers MGN_E_HIP.
 * Every mgn_group_* call below takes the arguments of the mgn_* call of the same name, hands that call to every worker, waits for all
 * of them and returns MGN_OK or the status of the rank that failed FIRST, with that rank's text behind "rank k: " in
 * mgn_group_last_error.  Inputs are host pointers that every rank reads in place (the nranks > 1 contract: GLOBAL arrays in, the
 * complete result on every rank).  Rank 0 writes the caller's output buffers (out, dxdt, d->out and d's counters, grads, *loss); the
 * other ranks write scratch the group owns.  grads of mgn_group_step and mgn_group_step_datapoint may also be device memory of devices[0].
 * The datapoint family (mgn_group_train_*, mgn_group_step_datapoint, mgn_group_datapoint_export) is the partitioned form of the calls of
 * the same names: mgn_group_train_norm_state reads rank 0's totals (all ranks hold the same bits) and restores the given ones on every
 * rank; for mgn_group_datapoint_export every rank writes its own, disjoint rows straight into the caller's host arrays, which come
 * back complete.
 * mgn_group_latents_checksum adds the ranks' sums in ascending rank order.
 * A rank that fails while its peers are inside a collective does not cost them MGN_COMM_TIMEOUT_S: the group raises the communicator's
 * abort flag the moment a rank returns an error, the peers leave with MGN_E_RCCL, and before the call returns the group replaces the
 * communicator with a fresh one: the group stays usable (graph, parameters and static inputs of the ranks are kept).
 * A group is no more thread-safe than a handle: one call in flight.  mgn_group_rank_handle lends rank k's handle for introspection
 * (mgn_partition_info, mgn_owned_nodes, mgn_halo_*, mgn_profile_*): no compute and no collective through it.
 * Refusals of mgn_group_create: MGN_E_ARG for nranks < 1, nranks > 64, NULL cfg / devices / out, a mix of MGN_DEVICE_NONE and devices;
 * MGN_E_UNSUPPORTED for n_edge_sets == 2 or ln_dims = MGN_LN_ALL with nranks > 1 (single-partition modes); whatever mgn_create
 * refuses.  nranks == 1 is a plain handle on a thread.                                                                            */
typedef struct mgn_group mgn_group;
int mgn_group_create(const mgn_config* cfg, int32_t nranks, const int32_t* devices /* [nranks] HIP ordinals; may repeat */, mgn_group** out);
void mgn_group_destroy(mgn_group* g);
const char* mgn_group_last_error(const mgn_group* g); /* g may be NULL: error of the last failed mgn_group_create */
mgn_handle* mgn_group_rank_handle(mgn_group* g, int32_t rank);
int mgn_group_set_params(mgn_group* g, const float* packed, size_t n);
int mgn_group_set_norms(mgn_group* g, const float* node_scale, const float* node_shift, const float* edge_scale, const float* edge_shift,
                        const float* out_scale, const float* out_shift);
int mgn_group_set_graph(mgn_group* g, int32_t N, int64_t E, const int32_t* senders, const int32_t* receivers, int32_t index_base,
                        const float* mesh_pos, int32_t pos_dim);
int mgn_group_set_static(mgn_group* g, const float* node_type_onehot, const float* ef_raw, const float* val_mask);
int mgn_group_forward(mgn_group* g, const float* nf, const float* ef, float* out);
int mgn_group_ode_step(mgn_group* g, const float* x, const float* node_type_onehot, const float* ef_raw, const float* val_mask, float* dxdt);
int mgn_group_rollout(mgn_group* g, mgn_rollout_desc* d);
int mgn_group_step(mgn_group* g, const float* nf, const float* ef, const float* target, const int32_t* mask, int64_t nmask,
                   int32_t mask_index_base, float* grads, size_t n_grads, float* loss);
int mgn_group_train_set_trajectory(mgn_group* g, const float* frames, int32_t T, const float* times, float dt,
                                   const float* node_type_onehot, const float* ef_raw);
int mgn_group_train_set_noise(mgn_group* g, const float* stddev, const uint8_t* noisy, uint64_t seed);
int mgn_group_train_online_norms(mgn_group* g, int32_t node_on, int32_t edge_on, int32_t out_on, double max_accumulations, float std_epsilon);
int mgn_group_train_norm_state(mgn_group* g, int32_t group, int32_t write, double* sum, double* sum_squares, double* count_and_calls);
int mgn_group_step_datapoint(mgn_group* g, int32_t datapoint, int32_t accumulate, const int32_t* mask, int64_t nmask,
                             int32_t mask_index_base, float* grads, size_t n_grads, float* loss);
int mgn_group_datapoint_export(mgn_group* g, int32_t datapoint, int32_t normalised, float* nf, float* ef, float* target);
/* Solver-based training (SolverTraining; MultipleShooting window by window) and the validation rollout on the partitioned mesh.  The
 * rank-handle symbols of the same names keep refusing a partitioned handle; these five reach the same drivers with partitions served.
 * Arguments are those of the namesake with GLOBAL host arrays (x, lambda, nf, ybar, gt, cont_target, val_mask, inflow mask and data,
 * sel: indices into the whole mesh's [N][O]); results are complete and in the caller's order (xbar, nfbar, dxdt, out, d->out,
 * mse_time through a row gather), the same bits on every rank, rank 0's returned.  nranks == 1: the plain call, the same bits.
 *   Each rank integrates and sweeps the rows it owns; every right-hand side and every VJP of the sweep exchanges halo rows as mgn_step
 *   does (mps forward exchanges, and mps reverse ones per VJP, each before the node MLP below is unwound); the solve runs eagerly.
 *   The adaptive controller's error norm is reduced over the ranks to the same bits, so every rank takes the same steps.
 *   Divisors are the whole mesh's: the save term of the loss and its seed use n_saves N O, mse_save N, val_loss n_sel (N O when
 *   n_sel == 0); a sel entry counts on the rank that owns its node, as often as it is listed; a rank that owns none of sel, or whose
 *   share of val_mask is zero, still takes part in every exchange.
 *   Finish, once per call: mgn_group_solver_grad* gathers every rank's DOUBLE gradient accumulator and its two loss sums (save terms,
 *   continuity term) and adds them in ascending rank order in double with one kernel on every rank; the gradient is rounded to fp32
 *   there, once.  mgn_group_rollout_eval folds the [n_saves][O] per-save sums and the val_loss numerator the same way.  mgn_group_ode_vjp
 *   and mgn_group_forward_vjp fold the fp32 gradient as mgn_step's finish does.  No floating-point atomics: bitwise repeatable.
 *   Memory is per rank: fixed-step Euler stores (K + 1) n_own O floats of states, Tsit5 6 n_own O floats per accepted step;
 *   mgn_solver_grad_opts.max_store_bytes bounds EACH rank's stored stage inputs, and stored_bytes, n_steps and the step record are
 *   rank 0's (the steps are the same on every rank, stored_bytes is rank 0's own 24 n_own O bytes per step).
 *   mgn_group_rollout_eval with d->out == NULL gathers and downloads nothing of [n_saves][N][O] on any rank.
 *   Every argument check (time grid, n_grads, fp32, one edge set, communicator, sel range) comes before the first collective; the
 *   status is the rank-handle call's for the same mistake.  A rank-local failure later (an allocation) releases the peers through the
 *   group's abort.  Not built: a group form of mgn_shooting_grad -- loop over the windows with mgn_group_solver_grad*; bf16, two edge sets and
 *   ln_dims = MGN_LN_ALL stay single-partition.                                                                                    */
int mgn_group_ode_vjp(mgn_group* g, const float* x, const float* node_type_onehot, const float* ef_raw, const float* val_mask,
                      const float* lambda, float* dxdt, float* xbar, float* grads, size_t n_grads);
int mgn_group_forward_vjp(mgn_group* g, const float* nf, const float* ef, const float* ybar, float* out, float* nfbar, float* grads,
                          size_t n_grads);
int mgn_group_solver_grad(mgn_group* g, mgn_rollout_desc* d, const float* gt, const float* loss_scale, const float* cont_target,
                          float cont_weight, float* grads, size_t n_grads, float* loss);
int mgn_group_solver_grad_tsit5(mgn_group* g, mgn_rollout_desc* d, mgn_solver_grad_opts* o, const float* gt, const float* loss_scale,
                                const float* cont_target, float cont_weight, float* grads, size_t n_grads, float* loss);
int mgn_group_rollout_eval(mgn_group* g, mgn_rollout_desc* d, mgn_rollout_eval_desc* e);
/* mgn_rollout_erk / mgn_rollout_eval_erk on the partitioned mesh: the same tableau and step mode on every rank, rank 0's counters back */
int mgn_group_rollout_erk(mgn_group* g, mgn_rollout_desc* d, const double* tab, int32_t adaptive);
int mgn_group_rollout_eval_erk(mgn_group* g, mgn_rollout_desc* d, mgn_rollout_eval_desc* e, const double* tab, int32_t adaptive);
int mgn_group_latents_randn(mgn_group* g, uint64_t seed);
int mgn_group_processor_steps_dev(mgn_group* g, int32_t nsteps);
int mgn_group_latents_checksum(mgn_group* g, double* sum_v, double* sum_e, double* sumsq_v, double* sumsq_e);
int mgn_group_synchronize(mgn_group* g);
/* Replica groups (a minibatch of datapoints split over devices that each hold the whole mesh) and the group forms of Adam and of the
 * resident parameters: seven more calls on the group, declared and documented in the file next to this one.                      */
#include "mgn_hip_replica.h"

/* ---- the benchmarked unit: nsteps processor steps on given latents -------------
 * v [N][L], e [E][L] in caller order, updated in place (host buffers).                          */
int mgn_processor_steps(mgn_handle* h, float* v, float* e, int32_t nsteps);

/* Device-resident variant: latents live in the engine (import/randn them first); nothing crosses
 * PCIe.  Enqueues 2*nsteps kernels (+1 projection) on the stream; with nranks > 1 (after mgn_comm_init) every rank calls
 * it and the halo exchange between the steps runs inside (see the multi-GPU section).          */
int mgn_latents_import(mgn_handle* h, const float* v, const float* e);   /* host, GLOBAL arrays   */
int mgn_latents_export(mgn_handle* h, float* v, float* e);               /* host, owned rows only */
int mgn_latents_randn(mgn_handle* h, uint64_t seed); /* N(0,1) keyed by GLOBAL node/edge id      */
int mgn_latents_checksum(mgn_handle* h, double* sum_v, double* sum_e, double* sumsq_v, double* sumsq_e);
int mgn_processor_steps_dev(mgn_handle* h, int32_t nsteps);

/* ---- fine-grained stages (multi-partition driver; each enqueues on the stream) ----------------
 * Order per forward:   enc -> [halo] -> for k: edge(k) -> node(k) -> [halo] -> ... -> dec
 * Order per processor: begin -> [halo] -> for k: edge(k) -> node(k) -> [halo]
 * [halo] = mgn_halo_pack -> exchange rows between ranks (RCCL all-to-all-v) -> mgn_halo_unpack.    */
int mgn_fwd_upload(mgn_handle* h, const float* nf, const float* ef); /* host GLOBAL arrays -> device local */
int mgn_fwd_encode(mgn_handle* h);
int mgn_proc_begin(mgn_handle* h);                      /* project P,Q of step 0 from current v     */
int mgn_proc_edge(mgn_handle* h, int32_t k);
int mgn_proc_node(mgn_handle* h, int32_t k, int32_t project_next); /* project_next: also emit P,Q of step k+1 */
/* Split form for overlapping the halo exchange (owned nodes are numbered boundary-first):
 *   phase 1: node MLP of step k on all nodes + projection (P,Q of step k+1; k = -1: of step 0) of the BOUNDARY tiles
 *   -> mgn_halo_pack + start the exchange ->
 *   phase 2: projection of the interior tiles     -> finish the exchange, mgn_halo_unpack.
 * phase 1 followed by phase 2 equals mgn_proc_node(h, k, 1) (k >= 0) or mgn_proc_begin (k = -1). */
int mgn_proc_node_phase(mgn_handle* h, int32_t k, int32_t phase);
/* The edge step split the same way (SURVEY.md 8e "interior edges while the halo is in flight, boundary edges after"):
 * edges whose sender is a halo node all lie in the first `boundary` 32-edge tiles of the receiver-sorted list (mesh edges
 * are two-way, so they end at boundary nodes, which are numbered first).  phase 1: tiles [boundary, total) -- needs no
 * exchanged row, may run before mgn_halo_unpack; phase 2: tiles [0, boundary).  phase 1 + phase 2 == mgn_proc_edge.   */
int mgn_proc_edge_phase(mgn_handle* h, int32_t k, int32_t phase);
int mgn_edge_boundary_tiles(const mgn_handle* h, int32_t set, int32_t* boundary, int32_t* total);
int mgn_fwd_decode(mgn_handle* h);
int mgn_fwd_download(mgn_handle* h, float* out);        /* host GLOBAL [N][O]; owned rows written   */
int mgn_halo_bytes_per_row(const mgn_handle* h);
int mgn_halo_pack(mgn_handle* h, void* send_dev);       /* device buffer, sum(send_rows) rows       */
int mgn_halo_unpack(mgn_handle* h, const void* recv_dev); /* device buffer, sum(recv_rows) rows     */

/* ---- measurement hooks ------------------------------------------------------------------------ */
/* Average device time (HIP events on the launch stream) of each kernel family since the last reset:
 * ms[0]=edge step, ms[1]=node step, ms[2]=encode, ms[3]=decode, ms[4]=halo pack/unpack; counts alike. */
int mgn_profile_enable(mgn_handle* h, int32_t on);
int mgn_profile_read(mgn_handle* h, double ms_avg[8], int64_t counts[8]);   /* slots: edge, node, encode, decode, halo, boundary edge tiles */

/* ---- data formats: host code, no handle -------------------------------------------
 * TFRecord framing + tf.train.Example decoding of the DeepMind MeshGraphNets datasets, as the reference reads them
 * through TFRecord.jl (read(path; channel_size) at src/dataset.jl:107-112; one Example per trajectory, consumed by
 * parse_data src/dataset.jl:61-75).  mgn_tfrecord_next: 1 = a record is loaded, 0 = end of file, < 0 = error
 * (CRC mismatch, truncation, malformed protobuf; text from mgn_tfrecord_error).  mgn_tfrecord_feature hands out the
 * payload of feature `key` of the current record: kind 1 = bytes_list (first value, what parse_data reinterprets by
 * meta.json's dtype), 2 = float_list (float32 array), 3 = int64_list (int64 array); the pointer stays valid until the
 * next mgn_tfrecord_next / close.  Unknown key -> MGN_E_ARG (KeyError on the Julia side).                        */
typedef struct mgn_tfrecord mgn_tfrecord;
int mgn_tfrecord_open(const char* path, int32_t verify_crc, mgn_tfrecord** out);
int mgn_tfrecord_next(mgn_tfrecord* r);
int mgn_tfrecord_feature_count(const mgn_tfrecord* r);
const char* mgn_tfrecord_feature_name(const mgn_tfrecord* r, int32_t i);
int mgn_tfrecord_feature(const mgn_tfrecord* r, const char* key, int32_t* kind, const void** data, int64_t* nbytes);
const char* mgn_tfrecord_error(const mgn_tfrecord* r);
void mgn_tfrecord_close(mgn_tfrecord* r);
uint32_t mgn_crc32c(const void* data, size_t n);   /* CRC-32C (Castagnoli) as used by the record framing */

#ifdef __cplusplus
}
#endif
#endif /* MGN_HIP_H */
