// Engine state shared by the C-ABI translation units (mgn_api.cpp: inference path, mgn_solve.cpp: the ODE solve drivers,
// mgn_train.cpp: step! and the reverse sweeps).
// Internal; the public boundary is include/mgn_hip.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <exception>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "../../include/mgn_hip.h"
#include "comm.h"
#include "graph_host.h"
#include "kernels.h"
#include "train.h"

namespace mgn {

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    hipError_t ensure(size_t n) {
        if (n <= bytes && p) return hipSuccess;
        release();
        if (n == 0) n = 16;
        hipError_t e = hipMalloc(&p, n);
        if (e == hipSuccess) bytes = n;
        return e;
    }
    template <typename T> T* as() const { return reinterpret_cast<T*>(p); }
};

// offsets (in floats) of one MLP inside the packed parameter vector: nl = hidden_layers + 1 Dense layers
constexpr int MAX_DENSE = 5;        // hidden_layers <= 4
struct MlpOff {
    size_t W[MAX_DENSE], b[MAX_DENSE], gamma = 0, beta = 0;
    int in = 0, out = 0, nl = 3;
    bool ln = false;
};
// offsets (floats, into wfrag) of the Dense layers after the first one of an MLP, for the GEN kernels (kernels.h GenMlp)
struct GenOff {
    size_t ch[4] = {0, 0, 0, 0}, tabs = 0;
};
// One L x L chunk of the network's weights as the tuned kernels see it: the offset (in elements) of each device copy of it, NONE
// where that copy is not built, and the power of two its fp16 pieces were multiplied by (1 without fp16 pieces).
//   frag         wfrag: fp32 fragment order, its t-major copy at + L L, its 16x16x4 copy at + 2 L L
//   sp32 / sp16  wsp: three bf16 pieces (WPackJob kinds 1 / 2) in the 32x32x16 / 16x16x32 fragment order
//   h32 / h16    wsp: two fp16 pieces of the chunk times `scale` (kinds 4 / 5) in the same two orders
//   bf           wbf: one bf16 copy (kind 3)
// Which copies a chunk gets is decided by its role and the configuration alone (mgn_api.cpp, pack_inference_weights):
//   frag: every chunk;  bf: processor chunks when dtype = MGN_BF16;  sp16, h16: processor chunks when L = 128 and hidden_layers = 2
//   (the 16-row kernels, both storage modes);  sp32, h32: the same in fp32 storage only (the 32-row kernels of split.hip; no h32 of
//   the second edge set's node-side chunks, which no kernel takes);  encoders and decoder: frag, and h32 under the same condition.
struct ChunkRef {
    static constexpr size_t NONE = ~(size_t)0;
    size_t frag = NONE, sp32 = NONE, sp16 = NONE, h32 = NONE, h16 = NONE, bf = NONE;
    float scale = 1.f;
};

enum Family { F_EDGE = 0, F_NODE, F_ENC, F_DEC, F_HALO, F_EDGE_BND, F_NFAM };   // F_EDGE_BND: boundary tiles of a split edge step

struct ProfRec {
    int fam;
    hipEvent_t a, b;
};

}  // namespace mgn

namespace mgn { struct TrainState; }
using mgn::DevBuf;
using mgn::MlpOff;
using mgn::GenOff;
using mgn::ChunkRef;
using mgn::ProfRec;
using mgn::LocalGraph;
using mgn::MAX_EDGE_SETS;

struct mgn_engine {
    // (fields use mgn:: types)

    mgn_config cfg{};
    std::string err;
    hipStream_t stream = nullptr;
    hipStream_t own_stream = nullptr;
    bool host_only = false;

    // parameters
    bool have_params = false;
    DevBuf d_params, d_wjobs;   // the RESIDENT parameter vector (what k_pack_weights and k_pack_train build every layout from, what mgn_adam_update rewrites) and the inference chunk list on the device
    std::vector<mgn::WPackJob> wjobs;   // (the list, kept for mgn_debug_pack_check)
    bool packed_ok = false;     // the kernels' weight layouts (wfrag, wsp, wbf) are those of `params`: mgn_set_params only stores the vector,
                                // the first compute call that reads them packs (a training loop -- set_params, step!, ... -- never does)
    std::vector<float> params;  // packed, host: always param_count long once parameters were set; its VALUES only through host_params()
    // Which copy of the parameter vector is authoritative.  mgn_set_params fills the host copy (d_params follows at the next pack:
    // params_dev_ok says whether it has); mgn_set_params_dev and mgn_adam_update write d_params and leave the host copy stale
    // (params_host_stale), which host_params() mends with one copy and one synchronisation -- as sync_norms_host does for the norms.
    bool params_dev_ok = false, params_host_stale = false;
    // Optimisers.Adam on d_params (mgn_adam_*): moments [param_count] each, beta_t = (beta1^t, beta2^t) in double as Optimisers keeps
    // it, the gradient's staging buffer for a caller whose gradient is host memory.  Independent of the parameters and of the graph.
    bool adam_ready = false;
    mgn_adam_desc adam{};
    double adam_beta_t[2] = {0.0, 0.0};
    DevBuf adam_m, adam_v, adam_g;
    MlpOff enc_node, dec;
    std::vector<MlpOff> pn;
    // the kernels' weight layouts: wfrag (fp32: all chunks + tables + small tensors, fragment order), wsp (16-bit pieces of the split
    // path, split.hip), wbf (bf16 storage); which chunk has a copy where: ChunkRef
    DevBuf wfrag, wsp, wbf;
    // One processor step.  e[q][i]: the edge MLP of set q in EdgeArgs::chunk order (0 W2, 1 W3, 2 W1 rows [2L, 3L): the e block);
    // n[i]: the node side in NodeArgs::chunk order -- 0 W2, 1 W3, 2 W1v = W1 rows [0, L), 3 W1a = rows [L, 2L) of the node MLP,
    // 4 WP, 5 WQ = W1 rows [0, L), [L, 2L) of the NEXT step's set-0 edge MLP (the projection; its bias in n_tabs[T_BQ]), and with two
    // edge sets 6 W1a of set 1 = rows [2L, 3L), 7 WP1, 8 WQ1 = the same projection onto set 1's edge MLP (bias in p1_tabs[T_BQ]).
    // *_tabs, *_gen: tables and the GEN kernels' chunk lists in wfrag (floats); *_b2pos = max(0, max b2) where fp16 pieces exist.
    struct StepChunks {
        ChunkRef e[MAX_EDGE_SETS][3], n[9];
        size_t e_tabs[MAX_EDGE_SETS], n_tabs, p1_tabs;
        GenOff e_gen[MAX_EDGE_SETS], n_gen;
        float e_b2pos[MAX_EDGE_SETS], n_b2pos;
    };
    std::vector<StepChunks> steps;   // [mps + 1]; [mps]: the "project only" pseudo-step of mgn_proc_begin -- step 0 with the projections onto step 0's own edge MLPs
    ChunkRef en[4], de[2];           // node encoder in EncNodeArgs::chunk order (0 W2, 1 W3, 2 WP, 3 WQ of step 0, set 0), decoder (0 W1, 1 W2)
    size_t en_tabs = 0, en_w1f = 0, de_tabs = 0, de_w3f = 0, de_b3 = 0;
    GenOff en_gen, de_gen;

    // norms (device): node scale/shift [Fn], edge [Fe], out [O]; null = identity
    DevBuf norms;
    std::vector<float> norms_host;   // the same affine maps on the host (the whole-array LayerNorm mode's mgn_ode_step builds its inputs there)
    bool have_nnorm = false, have_enorm = false, have_onorm = false;
    bool norms_host_stale = false;   // the device rewrote `norms` (online normalisers of mgn_step_datapoint): sync_norms_host before norms_host is read

    // graph
    bool have_graph = false;
    LocalGraph g;
    int32_t nsets = 1;
    int32_t ntiles_n = 0;
    DevBuf d_own_gid, d_send_idx;
    // per edge set: parameters, topology, latents (set 0 = the reference's mesh edges; set 1 = world edges)
    struct EdgeSetState {
        int32_t Fe = 0;
        MlpOff enc;
        std::vector<MlpOff> pe;
        ChunkRef ee[2];                       // edge encoder (0 W2, 1 W3)
        size_t ee_tabs = 0, ee_w1f = 0;
        GenOff ee_gen;
        int32_t ntiles_e = 0;
        bool have_ef = false;
        DevBuf d_snd, d_rcv, d_rowptr, d_edge_gid, d_ef;
        DevBuf Elat, AGG, CARRY, P, Q, elat0;
        DevBuf bP, bQ, bElat, bAGG, bCARRY;   // bf16 mode
        std::vector<int32_t> gs, gr;          // host copy of the global edge list (kept only with two sets: rebuilds)
        int32_t gbase = 0;
    } es[MAX_EDGE_SETS];

    // latents and I/O
    // bf16 mode (cfg.dtype == MGN_BF16): bf16 copies of the processor state (and weights: wbf); the fp32 V / Elat buffers
    // then only carry encoder output / decoder input
    DevBuf bV;
    // static per-trajectory RHS inputs (mgn_set_static): cached encoded edge latents
    bool have_static = false;
    DevBuf stage;     // device staging image of caller-order latents (import / export)
    DevBuf lnall_v, lnall_e;   // mgn_processor_steps_dev under ln_dims = MGN_LN_ALL: the resident latents as caller-order rows for the unfused driver
    DevBuf gwork, gout, gpos, gtype;   // device-side graph prologue (csrc/graph_dev.hip): scratch, outputs, positions, node types
    DevBuf d_stamps;  // diagnostic builds only
    DevBuf ode;       // native rollout: state, stages, frames, saves, Elat0
    std::vector<std::unique_ptr<DevBuf>> stage_store;   // mgn_solver_grad*: chunks of stored stage inputs, grown as steps are accepted, kept across calls
    const float* srcA_override = nullptr;  // rollout: encoder reads the node state from here instead of d_nfA
    const float* elat_src_override = nullptr;   // right-hand sides on small meshes: step 0's edge kernel reads the trajectory's encoded edge latents from here (EdgeArgs::ElatSrc) instead of a restore copy into Elat
    float* out_override = nullptr;         // rollout: decoder writes dx/dt here instead of d_out
    DevBuf V, d_nfA, d_nfB, d_out, d_mask, d_sum;
    int32_t in_wa = 0, in_wb = 0;
    bool have_mask = false;
    bool lnall_edges = false;        // ln_dims = MGN_LN_ALL: the encoded edges of the resident static inputs sit in the whole-array arena

    // hipGraph of one mgn_processor_steps_dev(nsteps) pass: small meshes are launch-bound (3 kernels per step).
    // State machine per invalidation: first call runs eagerly (warms per-kernel attributes), second captures.
    int32_t use_graph = 1;          // MGN_GRAPH=0 disables
    int32_t graph_nsteps = -1;      // nsteps the cached graph was captured for
    int32_t graph_warm = -1;        // nsteps of the last eager run since the last invalidation
    hipGraphExec_t graph_exec = nullptr;
    // hipGraph of the resident right-hand side (mgn_ode_step after mgn_set_static) on small meshes; same life cycle
    hipGraphExec_t rhs_exec = nullptr;
    bool rhs_warm = false;
    // the same for mgn_forward (its device buffers keep their addresses between calls)
    hipGraphExec_t fwd_exec = nullptr;
    bool fwd_warm = false;

    // communicator (mgn_comm_init): the halo exchange and the staged schedule run inside the library
    mgn::Comm* comm = nullptr;
    int32_t force_staged = 0;                 // MGN_FORCE_STAGED=1: staged schedule even at nranks == 1 (self-test)
    DevBuf halo_send, halo_recv, gath_s, gath_r;
    DevBuf fold_s, fold_r;                    // rank_fold_f64: this rank's doubles, then every rank's and the folded head
    std::vector<size_t> hx_sb, hx_so, hx_rb, hx_ro;   // per-peer byte counts / offsets of one exchange (rebuilt per graph)
    bool hx_ready = false;
    bool hx_direct = false;                   // rows are received straight into the halo block of P (one edge set)
    std::vector<int32_t> all_gid;             // [nranks][1 + max_own]: every rank's (n_own, own_gid...) for output gathers
    int32_t max_own = 0;
    bool in_local = false;                    // d_nfA / d_nfB / d_ef hold LOCAL rows (nranks > 1 uploads only what it owns)

    // training step (mgn_step): weights in training order, kept activations, scratch -- created on first use
    mgn::TrainState* train = nullptr;

    // mgn_shooting_grad: the companion engine solving B windows at once on B copies of this handle's graph (engine order, node offset
    // w N), one per pass size B, kept until the graph changes, with the generation of the parameters it holds; the call's staging
    uint64_t params_gen = 0;               // bumped by every mgn_set_params that changes the parameters
    struct ShootKid { int32_t b = 0; mgn_engine* e = nullptr; uint64_t params_gen = 0; bool params_set = false; bool latents = false; };   // latents: the inference latents exist (a solve asked for them; mgn_step_datapoints never does)
    std::vector<ShootKid> shoot_kids;      // at most two pass sizes (a group's full passes and its remainder)
    DevBuf shoot;
    bool companion = false;                // this is a companion: its training arena never sizes itself from the device's free memory

    // profiling
    bool prof = false;
    std::vector<ProfRec> recs;
    std::vector<hipEvent_t> event_pool;   // recycled by mgn_profile_read: creating events inside the timed region costs microseconds each
};


namespace mgn {

int fail(mgn_engine* h, int code, const char* fmt, ...);
int need(mgn_engine* h, bool params, bool graph, bool packed = true, bool lnall_ok = false);   // packed = false: the caller reads h->params only (training, get_params)
// Fn, Fe, Fe2, O <= L on the training kernels: the first width above L, or null; and the MGN_E_UNSUPPORTED of the training entry points
const char* width_over_L(const mgn_config& c, int* w);
int width_refuse(mgn_engine* h, const char* who);
int pack_inference_weights(mgn_engine* h);
// L x L chunk of W (row-major [K][ldw], rows kbase.., all L output columns) -> MFMA fragment order
void pack_chunk(float* dst, const float* W, int ldw, int kbase, int L);
void pack_chunk_tmajor(float* dst, const float* frag, int L);
void pack_chunk16(float* dst, const float* W, int ldw, int kbase);
// vector of L values (stride between consecutive features = stride) -> table fragment order
void pack_tab(float* dst, const float* vec, int L, int stride = 1);
// mgn_train.cpp: drop training-side state that depends on the parameters (what & 1), the graph (what & 2: the resident trajectory of
// mgn_train_set_trajectory goes with it) or the norms (what & 4: that trajectory's normalised edge rows); free it all
void train_invalidate(mgn_engine* h, int what);
void train_free(mgn_engine* h);
// mgn_config.ln_dims = MGN_LN_ALL (whole-array LayerNorm): the unfused forward (mgn_train.cpp)
int lnall_forward(mgn_engine* h, const float* nf, const float* ef, float* out);
int lnall_processor_steps(mgn_engine* h, float* v, float* e, int32_t nsteps);
int lnall_rhs_prepare(mgn_engine* h);                                              // binds the arena (may allocate / copy: outside of any capture)
int lnall_rhs_dev(mgn_engine* h, const float* srcA, float* out, bool reuse_edges);  // the right-hand side on resident inputs; launches only
// Solver-based training (mgn_solver_grad*, mgn_shooting_grad): the training-side checks and arena (train_prepare), and the reverse sweep
// over the stage inputs the forward loop stored (mgn_train.cpp).  Device arrays in the engine's order unless noted; the user's pointers
// are read with hipMemcpyDefault.  The method is data: its `stages` active stages s (those whose right-hand side is evaluated on a stage
// input of the step: all of them, less the FSAL stage; Euler: 1, Tsit5: 6), b[0 .. s) and A[j][i], 0-based
struct SolverSweep {
    int64_t K;                           // accepted steps
    const float* const* steps;           // [K] (host): step n's stored stage inputs z_{n,1 .. s}, [s][N][O] each
    const double* h;                     // [K] (host): the step sizes
    const float* xend;                   // [N][O]: x_K (continuity term)
    float* ybar;                         // scratch [s - 1][N][O]: ybar_2 .. ybar_s of the step being swept
    int32_t stages;                      // s, 1 .. 6
    const double* b;                     // [s]
    const double (*A)[7];                // [s][7]
    const float* saves;                  // [n_saves][N][O]: the solution at the save points
    const int64_t* save_step;            // [n_saves] (host): the step whose state each save is, non-decreasing
    int32_t n_saves;
    const float* gt;                     // [n_saves][N][O]
    const float* loss_scale;             // [O] or null
    const uint8_t* inflow;               // [N] or null
    const float* cont_target;            // [N][O] or null (continuity term on x_K)
    float cont_weight;
    const float* onehot; const float* ef_raw; const float* val_mask;   // the caller's, in the caller's order
    float* a; double* gacc; double* part;   // a = dL/dx (lam) [N][O]; scratch [n_params], [n_saves + 1][2][solver_adjoint_blocks]
    float* grads; float* loss;              // results (grads: host or device)
    // dense saves (MGN_TSIT5_DENSE_SAVES, Tsit5 only; theta null: every save is a state).  Save s with theta[s] >= 0 was interpolated inside
    // accepted step save_step[s] at that theta (save_step stays non-decreasing); its loss terms reach lam_n, kbar_{n,1 .. 6} and kbar_{n+1,1}
    // through k_tsit5_dense_adjoint, not through the adjoint launch of a state.
    const double* theta = nullptr;       // [n_saves] (host); < 0: the save is state save_step[s]
    const float* zend = nullptr;         // [N][O]: z_{K,1}, the input k_{K-1,7} was evaluated on (the extra VJP of a last step with such saves)
    float* dense = nullptr;              // scratch [7][N][O]: the step's sum of seeds, then W_1 .. W_6
    // mgn_shooting_grad (unset otherwise): the state holds windows of win_rows rows; the continuity weight per window (cw_win, device) replaces
    // cont_weight, the loss terms are added into lacc ([2][lacc_ld] doubles, launch_shoot_adjoint), every VJP adds to gacc (the caller zeroed
    // it), and nothing is finalised: the caller does that once for all passes
    const float* cw_win = nullptr; int64_t win_rows = 0;
    double* lacc = nullptr; int32_t lacc_ld = 0; double lscale = 0.0;
};
int solver_prepare(mgn_engine* h, size_t n_grads);
int erk_sweep(mgn_engine* h, const SolverSweep& S);

// mgn_api.cpp, for the solve drivers of mgn_solve.cpp.  Hidden: they were file-local before the drivers had a file of their own, and
// with default visibility these mgn:: functions would join the library's dynamic symbols
#pragma GCC visibility push(hidden)
int encode_impl(mgn_engine* h, bool use_norms, bool nodes = true, bool edges = true);
int decode_impl(mgn_engine* h, bool use_norms);
int run_processor(mgn_engine* h, int nsteps);
int upload_inputs(mgn_engine* h, const float* a, int wa, const float* b, int wb, const float* ef, bool engine_order = false);
bool elat_src_ok(mgn_engine* h);
void invalidate_static(mgn_engine* h);
int sync_norms_host(mgn_engine* h);    // norms_host <- norms where the device rewrote them (a copy of 2 (Fn + Fe + O) floats, blocking); else nothing
// The parameter vector's two copies (mgn_engine::params_dev_ok / params_host_stale).  host_params: the host copy, refreshed from the
// device first where that one is newer (one copy, blocking) -- every host reader of h->params' values goes through it.  dev_params: the
// resident device copy, uploaded from the host first where that one is newer (blocking only then: the upload reads pageable memory).
// set_params_resident: new values from src (host or device) into the resident copy on the handle's stream, with everything
// mgn_set_params invalidates; no comparison, no host work and, for a device source outside of captured inference graphs, no
// synchronisation.  params_changed_on_device: that invalidation alone (mgn_adam_update rewrote the resident copy in place).
int host_params(mgn_engine* h, const float** p);
int dev_params(mgn_engine* h, const float** p);
int set_params_resident(mgn_engine* h, const float* src, size_t n, const char* who);
int params_changed_on_device(mgn_engine* h);
bool is_device_pointer(const void* p);   // device (or managed) memory, as hipPointerGetAttributes sees it; plain host memory: false
size_t tile_floats(int64_t ntiles, int L);
int alloc_latents(mgn_engine* h);
int rebuild_graph(mgn_engine* h, int32_t N, const EdgeList* sets, const float* mesh_pos, int32_t pos_dim, bool keep_owner, const char* who,
                  const int32_t* owner_in = nullptr, int renumber = -1);
int need_comm(mgn_engine* h, const char* who);
int gather_rows_global(mgn_engine* h, const float* local_dev, int W, float* out);
int rank_fold_f64(mgn_engine* h, double* head, int64_t nhead, const double* acc, int64_t n, float* out);
bool is_bf16(const mgn_engine* h);
void shoot_release(mgn_engine* h);     // mgn_solve.cpp: drops mgn_shooting_grad's companions and staging
// mgn_solve.cpp: the cached companion engine of B block-diagonal copies of h's graph (mgn_shooting_grad: inference = true; mgn_step_datapoints: false)
int companion_engine(mgn_engine* h, int32_t B, const char* who, bool inference, mgn_engine** out);
// The drivers behind mgn_ode_vjp, mgn_forward_vjp (mgn_train.cpp), mgn_solver_grad, mgn_solver_grad_tsit5 and mgn_rollout_eval
// (mgn_solve.cpp): the public symbols' checks and work, with `partitions` saying whether a partitioned handle (nranks > 1) is served.
// The rank-handle symbols pass false and keep their refusals; mgn_group_* (mgn_group.cpp) passes true.  On a partitioned call every
// check comes before the first collective; inputs are the GLOBAL host arrays, results the complete ones on every rank.
int ode_vjp_run(mgn_engine* h, const float* x, const float* node_type_onehot, const float* ef_raw, const float* val_mask, const float* lambda,
                float* dxdt, float* xbar, float* grads, size_t n_grads, bool partitions);
int forward_vjp_run(mgn_engine* h, const float* nf, const float* ef, const float* ybar, float* out, float* nfbar, float* grads, size_t n_grads,
                    bool partitions);
int solver_grad_run(mgn_engine* h, mgn_rollout_desc* d, mgn_solver_grad_opts* o, int32_t solver, const float* gt, const float* loss_scale,
                    const float* cont_target, float cont_weight, float* grads, size_t n_grads, float* loss, bool partitions);
// (tab: mgn_rollout_eval_erk's tableau, checked here before anything else, and its step mode; null: the solver d->solver names)
int rollout_eval_run(mgn_engine* h, mgn_rollout_desc* d, mgn_rollout_eval_desc* e, bool partitions, const double* tab = nullptr, int32_t adaptive = 0);
int solver_prepare_partitions(mgn_engine* h, const char* who, size_t n_grads);   // solver_prepare for a call that serves partitions too
// mgn_train.cpp, for mgn_group_step_datapoints (mgn_group.cpp).
// step_datapoints_check: every refusal of mgn_step_datapoint (share == 1) or mgn_step_datapoints (share > 1) for a list of B datapoints
// of which this handle takes at most `share`, with that call's status, in its order; host work only -- nothing is launched, packed or
// allocated on the device, no collective is entered.
// datapoint_accumulate: datapoint_norms(h, t, true, h->stream), the online normalisers' accumulation of one datapoint (what
// mgn_step_datapoint(s) runs per entry with accumulate != 0); the handle has passed step_datapoints_check.
int step_datapoints_check(mgn_engine* h, const char* who, const int32_t* datapoints, int32_t B, int32_t share, const int32_t* mask, int64_t nmask,
                          int32_t mask_index_base, size_t n_grads);
int datapoint_accumulate(mgn_engine* h, int32_t t);
#pragma GCC visibility pop

#define HIPCHK(h, expr)                                                                              \
    do {                                                                                             \
        hipError_t _e = (expr);                                                                      \
        if (_e != hipSuccess)                                                                        \
            return mgn::fail(h, _e == hipErrorOutOfMemory ? MGN_E_OOM : MGN_E_HIP, "%s failed: %s (%s:%d)", #expr, \
                             hipGetErrorString(_e), __FILE__, __LINE__);                             \
    } while (0)

// The one place a launch sequence becomes a hipGraph: `launches` is issued under stream capture, the graph instantiated into `exec` and
// launched.  A stream that cannot be captured, a failed capture or a failed instantiation leave exec null and turn graph replay off
// for the handle (use_graph = 0: eager from here on); the sequence's own error is returned, otherwise it runs eagerly.
template <typename F>
int capture_and_launch(mgn_engine* h, hipStream_t st, hipGraphExec_t& exec, F&& launches) {
    exec = nullptr;
    if (hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) != hipSuccess) {
        (void)hipGetLastError();
        h->use_graph = 0;
        return launches();
    }
    hipGraph_t graph = nullptr;
    const int rc = launches();
    const bool ok = hipStreamEndCapture(st, &graph) == hipSuccess && rc == MGN_OK && graph &&
                    hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) == hipSuccess;
    if (graph) (void)hipGraphDestroy(graph);
    if (!ok) {
        exec = nullptr;
        h->use_graph = 0;
        return rc != MGN_OK ? rc : launches();
    }
    HIPCHK(h, hipGraphLaunch(exec, st));
    return MGN_OK;
}
// Small meshes: a launch sequence over buffers with fixed addresses runs eagerly once (per-kernel attributes are set outside of any
// capture), is captured on the next call and replayed afterwards.  graphable: the caller's size rule, with use_graph, no profiling and
// a stream other than the legacy NULL stream (mgn_set_stream(h, NULL)), which cannot be captured.
template <typename F>
int run_graphed(mgn_engine* h, hipStream_t st, bool graphable, hipGraphExec_t& exec, bool& warm, F&& launches) {
    if (graphable && exec) {
        HIPCHK(h, hipGraphLaunch(exec, st));
        return MGN_OK;
    }
    if (!graphable || !warm) {
        warm = true;
        return launches();
    }
    return capture_and_launch(h, st, exec, launches);
}

}  // namespace mgn

// No C++ exception crosses the C ABI (a Julia or C host would see std::terminate): every entry point is a function-try-block.
#define MGN_CATCH(h)                                                                                              \
    catch (const std::bad_alloc&) { return mgn::fail(h, MGN_E_OOM, "%s: host allocation failed", __func__); }     \
    catch (const std::exception& mgn_ex_) { return mgn::fail(h, MGN_E_ARG, "%s: %s", __func__, mgn_ex_.what()); }             \
    catch (...) { return mgn::fail(h, MGN_E_ARG, "%s: unknown C++ exception", __func__); }
#define MGN_CATCH_SIZE catch (...) { return 0; }
