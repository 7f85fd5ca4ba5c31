// mgn_step: the training step GraphNetCore.step!(mgn, graph, target, mask, mse_reduce) of the reference
// (src/strategies.jl:418-422; gradients applied at src/MeshGraphNets.jl:370-378) behind the C ABI.
// Host orchestration only -- weights repacked into training order (forward and transposed chunks), an arena of kept
// activations, kernel sequencing; all arithmetic is in train.hip.  No CPU compute path.
#include <algorithm>
#include <climits>
#include <cstring>
#include <numeric>

#include "engine_internal.h"
#include "train.h"
#include "launch.hpp"

namespace mgn {

namespace {

// The training kernels (train.hip) run ONE shape: Dense - ReLU - Dense - ReLU - Dense (+ LayerNorm, + residual), the reference's
// default hidden_layers = 2.  Other depths are expressed in that shape with identity slots, exactly (an identity product of an
// fp32 row is that row; ReLU of a value that is already a ReLU output is that value, and its mask in the reverse pass is the
// same mask):
//   hidden_layers = 1:  [D0, I, D1]
//   hidden_layers = 3:  [D0, I, I] -> [D1, D2, D3]        (the first block's output is ReLU(z0): no LayerNorm, no residual)
//   hidden_layers = 4:  [D0, D1, I] -> [D2, D3, D4]
// One such launch unit with its device offsets (floats into TrainState::w) in training order:
constexpr int LNSUM_GROUPS = 64;   // first-level groups of the in-kernel LayerNorm-parameter sums
// What one launch unit adds to its weight-gradient launch and to the reduction behind it: dW3, dW2 and up to three blocks of dW1 (the
// inputs of an MLP, or the e block and the two per-node blocks of a factored edge MLP), a column-sum job each for dgamma and dbeta where
// the backward kernel wrote GT / GXH rows; the reduction adds db3, db2, db1 and the two LayerNorm sums, from jobs or from LNSUM.
constexpr int UNIT_W_JOBS = 5;
static_assert(WGRAD_MAX_JOBS == UNIT_W_JOBS + 2, "a weight-gradient launch holds one unit's weight jobs and its two LayerNorm column sums");
static_assert(REDUCE_MAX_JOBS == UNIT_W_JOBS + 3 + 2, "a reduction holds one unit's weight blocks, its three biases, dgamma and dbeta");

struct TrainBlock {
    int nin = 1;                 // L-wide layer-1 input blocks
    int in_rows = 0;             // rows of W1 that exist (< L for the encoders: zero-padded chunk)
    size_t W1[3] = {0, 0, 0}, W2 = 0, W3 = 0, W2T = 0, W3T = 0, tabs = 0;
    size_t W1T[3] = {0, 0, 0};
    bool has_w1t = false, ln = false;
    long gW[3] = {-1, -1, -1}, gb[3] = {-1, -1, -1};   // packed-parameter offsets of the three slots (-1: identity slot, nothing to learn)
    long ggamma = -1, gbeta = -1;
    int out_cols = 0;            // columns of slot 3 that exist (decoder: O)
};
struct TrainMlp {
    int nblk = 1;
    TrainBlock b[2];
    int lnslot = -1;             // whole-array LayerNorm (ln_dims = MGN_LN_ALL): which (mean, rden, kappa) slot of the arena belongs to this MLP
};
// kept activations of one MLP instance: per block H1, H2, Y (arena offsets)
struct Acts { size_t h[2][3] = {{0, 0, 0}, {0, 0, 0}}; };

}  // namespace

struct TrainState {
    bool packed = false, graph_ready = false;
    bool factored[MAX_EDGE_SETS] = {false, false};   // edge MLPs with a factored first layer (P = v W1s, Q = v W1r per node): large meshes
    bool recompute = false;      // some processor steps keep only their inputs; their H1 / H2 / Y are recomputed in the reverse pass
    int keep_steps = 0;          // the LAST keep_steps processor steps store H1 / H2 / Y (all of them when !recompute)
    bool kept(int k, int mps) const { return k >= mps - keep_steps; }
    int nblk = 1;                // launch units per MLP (2 for hidden_layers 3, 4)
    DevBuf w;                    // training-order weights
    DevBuf pk_tabs, pk_jobs, pk_max;   // what k_pack_train builds them from, beside the resident parameter vector (mgn_engine::d_params): the units' table descriptions, the chunk list
    bool pk_described = false;         // ... which follow from the configuration alone: formed and uploaded once (pack_describe)
    int pk_njobs = 0;
    // enc-node, enc-edge (per set), per step: edge (per set), node; decoder
    TrainMlp m_en, m_de, m_ee[MAX_EDGE_SETS];
    std::vector<TrainMlp> m_pe[MAX_EDGE_SETS], m_pn;
    DevBuf arena, idx, grads, target, mask, loss;
    std::vector<int32_t> g2l, mask_host;       // renumbered graph: caller's node id -> engine row; the mapped mask of the call
    std::vector<int32_t> mask_seen;            // the (host) mask the device copy was made from, as the caller gave it
    bool mask_valid = false;
    int32_t mask_base = 0;
    // whole-array LayerNorm mode (lnall_*): its own small arena (no kept activations), the edge gids as int32
    DevBuf la, la_idx;
    bool la_ready = false;
    size_t arena_floats = 0;
    // arena offsets (floats)
    size_t nf_raw, nf_pad, ef_raw[MAX_EDGE_SETS], ef_pad[MAX_EDGE_SETS], V0, Enew;
    Acts a_en, a_de, a_ee[MAX_EDGE_SETS];
    std::vector<Acts> a_pe[MAX_EDGE_SETS], a_pn;
    std::vector<size_t> Ek[MAX_EDGE_SETS], Vk, agg[MAX_EDGE_SETS];
    static constexpr int GSETS = 4;   // gradient-buffer sets: the weight gradients of unit i run beside the backward of units i+1 .. i+3 (8, 16 and 40 sets measured slower)
    int gsets = 1;                    // sets allocated for the current graph (GSETS on small meshes, else 1: no overlap)
    size_t GT[GSETS], GXH[GSETS], GY[GSETS], GZ2[GSETS], GZ1[GSETS];
    size_t GXs, GXr, GXB, gV[2], gE[MAX_EDGE_SETS][2], gAgg[MAX_EDGE_SETS], Gout, gNF, io, ptmp, pw, pb;
    size_t Pn, Qn, SGs, SGr;     // factored first layer: per-node projections (forward) and summed GZ1 rows (backward)
    // whole-array LayerNorm in the training step: per-MLP statistics of the forward (64 floats each), the double partials of the two
    // reductions, (m1, m2) of the pullback
    size_t lnstats = 0, lnpart = 0, lnm = 0;
    bool need_gt = true;              // GT / GXH are full arrays (else 64-float stubs: every LayerNorm'd unit runs with LNSUM)
    size_t lnsum = 0, lnsum2 = 0;     // per-block LayerNorm-parameter sums of the streaming backward kernel and their first-level reduction (TrainBwdArgs::LNSUM)
    int size_cus = 0;                 // train_size_cus() the arena was laid out for: the launches decide by the same count (train_prepare lays it out again when the test CU count changed)
    int64_t wg_rpb_last = 0, wg_rpb_node = 0, wg_rpb_edge[MAX_EDGE_SETS] = {0, 0};   // rows per block of the last weight-gradient launch unit, of the processor's node MLP and of its edge MLPs (mgn_debug_train_regime)
    size_t segcarry = 0;              // carry rows of the fused aggregation (2 per edge tile; TrainFwdArgs::SEG_CARRY)
    // weight gradients + their reductions go to a second stream (small meshes leave most of the chip idle during k_mlp_bwd)
    hipStream_t aux = nullptr;
    hipEvent_t ev_bwd = nullptr, ev_wg[GSETS] = {};   // ev_wg[i]: the weight gradients of the unit in buffer set i have run
    // hipGraph replay of the two launch sequences over fixed buffers (small meshes): [0] forward, [1] backward of mgn_step,
    // [2] backward of mgn_ode_vjp (it also produces the input gradient).  Eager once, captured on the next call.
    hipGraphExec_t exec[3] = {nullptr, nullptr, nullptr};
    bool warm[3] = {false, false, false};
    const void* exec_arena = nullptr; const void* exec_w = nullptr;
    void drop_graphs() {
        for (int i = 0; i < 3; ++i) {
            if (exec[i]) (void)hipGraphExecDestroy(exec[i]);
            exec[i] = nullptr;
            warm[i] = false;
        }
    }
    ~TrainState() {
        drop_graphs();
        if (ev_bwd) (void)hipEventDestroy(ev_bwd);
        for (hipEvent_t e : ev_wg) if (e) (void)hipEventDestroy(e);
        if (aux) (void)hipStreamDestroy(aux);
    }
    // idx buffer (int32), per edge set: egid32 [E], perm_s [E], rowptr_s [N + n_halo + 1] (halo rows send, too)
    size_t i_egid[MAX_EDGE_SETS] = {0, 0}, i_perm[MAX_EDGE_SETS] = {0, 0}, i_rowptr_s[MAX_EDGE_SETS] = {0, 0};
    // Partitioned mesh (nranks > 1).  The forward exchange packs the owned boundary rows of v by the send index into hx_send and unpacks
    // hx_recv into the halo rows; the reverse one sends the halo rows of the gradient as they lie and adds what arrives to the owners'
    // rows through a CSR over the send index (idx buffer: acc_row [n_acc], acc_ptr [n_acc + 1], acc_pos [rows sent]).  Per-peer bytes /
    // offsets of the owned-row side (own) and of the halo side (halo) of either direction.  fin_*: one rank's part of the finish
    // (train.h: rank_sum_stride), all ranks' parts, the summed loss numerator.
    DevBuf hx_send, hx_recv, fin_s, fin_r, fin_loss;
    std::vector<size_t> hx_own_b, hx_own_o, hx_halo_b, hx_halo_o;
    size_t i_acc_row = 0, i_acc_ptr = 0, i_acc_pos = 0;
    int32_t n_acc = 0;
    int64_t mask_n = 0;          // entries of the device mask: the whole mask, on a partition the entries this rank owns
    // mgn_step_datapoint: the trajectory of mgn_train_set_trajectory, resident in the engine's node order, and the noise settings.
    // Dropped with the graph (train_invalidate & 2); mgn_set_params and mgn_set_norms leave it alone.
    struct Trajectory {
        bool have = false;
        int32_t T = 0;
        DevBuf frames, onehot, ef_raw;   // [T][N][O], [N][Fn - O] in the engine's node order; [E][Fe] in the caller's edge order (as ef_pad holds it)
                                         // A partition keeps the rows it owns: N = n_own, and its e_local edges in the ENGINE's order (as its ef_pad holds them)
        std::vector<float> delta;        // [T - 1]: dt, or times[t + 1] - times[t]
        bool noise = false, some_nodes = false;
        DevBuf stddev, noisy;            // [O]; [N] 0/1 in the engine's order (some_nodes)
        uint64_t seed = 0;
        bool ef_pad_ok = false;          // the arena's ef_pad[0] holds this trajectory's edge features under the norms as they stand
        uint64_t ef_gen = 0;             // bumped when the trajectory or the edge normaliser changes: what a companion's replicated edge rows were built from (Batch::ef_gen)
        bool ef_sums_ok = false;         // ef_sums holds ef_raw's column sums
        DevBuf ef_sums;                  // [2][Fe] doubles: what one accumulation of ef_raw adds (mgn_feature_stats' sums, formed once)
        DevBuf work;                     // accumulating steps: cur and d [N][O] each in the caller's order (a partition: its rows, the engine's order), then launch_col_stats' partials of both
        DevBuf xsum;                     // a partition's sums on their way to the peers: this rank's [cur | d] ([2][O] each) and its ef_raw's [2][Fe], then every rank's of either
        void drop() {
            have = false; T = 0; noise = some_nodes = false; ef_pad_ok = ef_sums_ok = false;
            ++ef_gen;
            delta.clear();
            for (DevBuf* b : {&frames, &onehot, &ef_raw, &stddev, &noisy, &ef_sums, &work, &xsum}) b->release();
        }
    } traj;
    // The online normalisers (GraphNetCore NormaliserOnline) of mgn_train_online_norms: group 0 the node state columns, 1 the edge
    // features, 2 the output.  They outlive graphs and trajectories, like the normalisers of the reference's model.
    struct OnlineGroup {
        bool online = false, dirty = false;   // dirty: the totals were restored; the maps follow at the next datapoint
        double count = 0.0, calls = 0.0, max_acc = 1e6;
        float eps = 1e-8f;
    } on[3];
    DevBuf on_totals;            // doubles [node sum, sum of squares (O each) | edge (Fe each) | output (O each)]
    // mgn_step_datapoints, on the companion of B copies (engine_internal.h: companion_engine) -- the parent's state holds the trajectory
    // and the normalisers, this one the batch: whether ef_pad[0] holds the parent trajectory's normalised edge rows B times and from which
    // Trajectory::ef_gen (a new arena resets ef_ok: prepare_graph), the parent's node map for the mask (a renumbered parent), and the
    // fold's result [loss_0 .. loss_{B-1} | mean].  The per-copy loss partials live in `loss`, the mask in `mask`.
    struct Batch {
        bool ef_ok = false;
        uint64_t ef_gen = 0;
        std::vector<int32_t> g2l;
        DevBuf out;
    } batch;
};

void train_invalidate(mgn_engine* h, int what) {
    if (!h || !h->train) return;
    if (what & 1) h->train->packed = false;
    if (what & 2) { h->train->graph_ready = false; h->train->la_ready = false; h->train->traj.drop(); }
    if (what & 4) { h->train->traj.ef_pad_ok = false; ++h->train->traj.ef_gen; }
}

void train_free(mgn_engine* h) {
    if (!h) return;
    delete h->train;
    h->train = nullptr;
}

namespace {

// The training layouts from the resident parameter vector.  What they are built FROM -- the ~300 chunk jobs, the description of every
// launch unit's tables, the offsets in TrainMlp -- depends on the configuration alone, so it is formed once per handle and kept on the
// device (pack_describe); a re-pack, which a training loop needs after every optimiser update, is the jobmax memset and the pack
// launches: no host pass over the parameters, no upload of them unless the host copy is the newer one (mgn_set_params: dev_params), no
// synchronisation.  Both doors for parameters end in the same buffer and the same kernels: the same bits.
int pack_describe(mgn_engine* h) {
    // an encoder's first layer is ONE block of at most L rows below (nin = m.in / L is the processor MLPs' 2 L and 3 L), the decoder's
    // last layer at most L columns: no caller comes here with a wider configuration (train_prepare and mgn_create's MGN_LN_ALL
    // check refuse it first); should one ever, it is turned away before a job is described
    if (int rc = width_refuse(h, "the training weight layout")) return rc;
    TrainState& T = *h->train;
    const mgn_config& c = h->cfg;
    const int L = c.L;
    const size_t CH = (size_t)L * L;
    size_t fsz = 0;                                   // floats of the packed buffer T.w
    std::vector<PackJob> jobs;
    std::vector<PackTab> tabs;                        // one per launch unit
    // rows [r0, r0 + nr) x cols [0, nc) of the matrix at parameter offset src (leading dimension ldw; src < 0: the identity), zero-padded
    // to L x L; transposed on request
    // L = 128: every chunk also as two fp16 pieces times a power of two that puts its largest entry into [2^14, 2^15) (split_common.hpp;
    // the streaming kernels of large launches compute on them), at + 2 CH, and 1 / that power at + 3 CH
    const bool pieces = L == 128;
    auto block = [&](long long src, int ldw, int r0, int nr, int nc, bool transpose) {
        const size_t off = fsz;
        fsz += pieces ? 3 * CH + 4 : 2 * CH;          // fragment order, then the t-major copy (cooperative kernels) at + CH
        const float sc = pieces ? 1.f : 0.f;          // (> 0: pieces wanted; their scale is found on the device, k_pack_absmax)
        jobs.push_back({(long long)off, src, ldw, r0, nr, nc, transpose ? 1 : 0, 0, sc});
        return off;
    };
    const size_t ident = block(-1LL, 0, 0, 0, 0, false);   // (its own transpose)
    auto build = [&](const MlpOff& m, bool need_input_grad) {
        TrainMlp t;
        const int nd = m.nl;                          // Dense layers: hidden_layers + 1
        int plan[2][3] = {{0, 1, 2}, {-1, -1, -1}};
        t.nblk = nd <= 3 ? 1 : 2;
        if (nd == 2) { plan[0][1] = -1; plan[0][2] = 1; }
        if (nd == 4) { plan[0][1] = plan[0][2] = -1; plan[1][0] = 1; plan[1][1] = 2; plan[1][2] = 3; }
        if (nd == 5) { plan[0][2] = -1; plan[1][0] = 2; plan[1][1] = 3; plan[1][2] = 4; }
        for (int bi = 0; bi < t.nblk; ++bi) {
            TrainBlock& b = t.b[bi];
            const int d0 = plan[bi][0], d1 = plan[bi][1], d2 = plan[bi][2];
            const bool last = bi == t.nblk - 1;
            b.nin = (bi == 0 && m.in >= L) ? m.in / L : 1;
            b.in_rows = (bi == 0 && m.in < L) ? m.in : L;
            b.has_w1t = need_input_grad || bi > 0;    // (a second block always hands its input gradient to the first)
            for (int j = 0; j < b.nin; ++j) {
                b.W1[j] = block((long long)m.W[d0], L, j * L, b.in_rows, L, false);
                if (b.has_w1t) b.W1T[j] = block((long long)m.W[d0], L, j * L, b.in_rows, L, true);
            }
            b.gW[0] = (long)m.W[d0]; b.gb[0] = (long)m.b[d0];
            if (d1 >= 0) {
                b.W2 = block((long long)m.W[d1], L, 0, L, L, false);
                b.W2T = block((long long)m.W[d1], L, 0, L, L, true);
                b.gW[1] = (long)m.W[d1]; b.gb[1] = (long)m.b[d1];
            } else b.W2 = b.W2T = ident;
            b.out_cols = L;
            if (d2 >= 0) {
                b.out_cols = d2 == nd - 1 ? m.out : L;
                b.W3 = block((long long)m.W[d2], b.out_cols, 0, L, b.out_cols, false);
                b.W3T = block((long long)m.W[d2], b.out_cols, 0, L, b.out_cols, true);
                b.gW[2] = (long)m.W[d2]; b.gb[2] = (long)m.b[d2];
            } else b.W3 = b.W3T = ident;
            b.ln = last && m.ln;
            // tables: biases (zero behind an identity slot), LayerNorm parameters of the last block
            const size_t off = fsz;
            fsz += (size_t)T_COUNT * L;
            jobs.push_back({(long long)off, (long long)tabs.size(), 0, 0, 0, 0, 0, 1, 0.f});
            PackTab tb{{-1, -1, -1, -1, -1}, {0, 0, 0, 0, 0}, 0.f, 0.f};
            tb.src[T_B1] = (long long)m.b[d0]; tb.cnt[T_B1] = L;
            if (d1 >= 0) { tb.src[T_B2] = (long long)m.b[d1]; tb.cnt[T_B2] = L; }
            if (d2 >= 0) { tb.src[T_B3] = (long long)m.b[d2]; tb.cnt[T_B3] = b.out_cols; }
            if (b.ln) {
                tb.src[T_GAMMA] = (long long)m.gamma; tb.cnt[T_GAMMA] = L;
                tb.src[T_BETA] = (long long)m.beta; tb.cnt[T_BETA] = L;
                b.ggamma = (long)m.gamma; b.gbeta = (long)m.beta;
            }
            tb.eps_in = c.ln_mode == MGN_LN_STD_EPS ? 0.f : 1e-5f;          // (eps_in, eps_out) of the LayerNorm variant
            tb.eps_out = c.ln_mode == MGN_LN_STD_EPS ? 1e-5f : 0.f;         // (frag.hpp: ln_rstd_at; both are trained)
            tabs.push_back(tb);
            b.tabs = off;
        }
        return t;
    };
    T.nblk = c.hidden_layers >= 3 ? 2 : 1;
    T.m_en = build(h->enc_node, true);                // input gradient: mgn_ode_vjp (d f / d x)
    T.m_pn.clear();
    for (int q = 0; q < h->nsets; ++q) {
        T.m_ee[q] = build(h->es[q].enc, false);
        T.m_pe[q].clear();
        for (int k = 0; k < c.mps; ++k) T.m_pe[q].push_back(build(h->es[q].pe[k], true));
    }
    for (int k = 0; k < c.mps; ++k) T.m_pn.push_back(build(h->pn[k], true));
    T.m_de = build(h->dec, true);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, T.w.ensure(fsz * 4));
    HIPCHK(h, T.pk_tabs.ensure(tabs.size() * sizeof(PackTab)));
    HIPCHK(h, T.pk_jobs.ensure(jobs.size() * sizeof(PackJob)));
    HIPCHK(h, T.pk_max.ensure(jobs.size() * sizeof(unsigned)));
    HIPCHK(h, T.grads.ensure(h->params.size() * 4));
    HIPCHK(h, hipMemcpyAsync(T.pk_tabs.p, tabs.data(), tabs.size() * sizeof(PackTab), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(T.pk_jobs.p, jobs.data(), jobs.size() * sizeof(PackJob), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));       // (jobs / tabs are locals: their copies must have left the host)
    T.pk_njobs = (int)jobs.size();
    T.pk_described = true;
    return MGN_OK;
}

int pack_training_weights(mgn_engine* h) {
    TrainState& T = *h->train;
    if (!T.pk_described)
        if (int rc = pack_describe(h)) return rc;
    const float* dp = nullptr;
    if (int rc = dev_params(h, &dp)) return rc;
    HIPCHK(h, launch_pack_train(h->cfg.L, T.pk_jobs.as<PackJob>(), T.pk_njobs, dp, T.pk_tabs.as<PackTab>(), T.pk_max.as<unsigned>(), T.w.as<float>(), h->stream));
    T.packed = true;
    return MGN_OK;
}

int prepare_graph(mgn_engine* h) {
    TrainState& T = *h->train;
    const LocalGraph& g = h->g;
    const int L = h->cfg.L, mps = h->cfg.mps, S = h->nsets, NB = T.nblk;
    const bool part = g.nranks > 1;
    // NT: rows of every node array -- the owned rows, then the halo rows that local senders index (V_k, P / Q, the gradients w.r.t. v).
    // Launches over nodes cover the N owned rows unless they say otherwise.  A partition stages the caller's GLOBAL arrays: NG, EG rows.
    const int64_t N = g.n_own, NT = N + g.n_halo, NG = part ? g.N : N;
    const size_t NL = (size_t)(NT > 0 ? NT : 1) * L;
    size_t EL[MAX_EDGE_SETS] = {0, 0}, ELmax = 0;
    int64_t Emax = 0;
    // index arrays per set: edge_gid as int32, sender CSR over the receiver-sorted edge list
    std::vector<int32_t> ix;
    for (int q = 0; q < S; ++q) {
        const EdgeTopo& t = g.set[q];
        const int64_t E = t.e_local;
        if ((int64_t)t.snd.size() != E || (int64_t)t.edge_gid.size() != E)
            return fail(h, MGN_E_STATE, "the training step needs the host copy of the edge lists: install the graph with mgn_set_graph / mgn_set_edge_set");
        EL[q] = (size_t)(E > 0 ? E : 1) * L;
        ELmax = std::max(ELmax, EL[q]);
        Emax = std::max(Emax, E);
        const size_t base = ix.size();
        ix.resize(base + (size_t)2 * E + NT + 1, 0);
        T.i_egid[q] = base;
        T.i_perm[q] = base + E;
        T.i_rowptr_s[q] = base + 2 * E;
        for (int64_t i = 0; i < E; ++i) ix[T.i_egid[q] + i] = (int32_t)t.edge_gid[i];
        int32_t* rp = ix.data() + T.i_rowptr_s[q];
        for (int64_t i = 0; i < E; ++i) ++rp[t.snd[i] + 1];
        for (int64_t n = 0; n < NT; ++n) rp[n + 1] += rp[n];
        std::vector<int32_t> cur(rp, rp + NT);
        for (int64_t i = 0; i < E; ++i) ix[T.i_perm[q] + cur[t.snd[i]]++] = (int32_t)i;   // stable: ascending edge position
    }
    T.n_acc = 0;
    if (part) {   // the owners' side of the reverse exchange: positions of the receive buffer (== of the send index) grouped by owned row, ascending
        const int P = g.nranks;
        const int64_t ns = (int64_t)g.send_idx.size();
        std::vector<int32_t> order((size_t)ns);
        std::iota(order.begin(), order.end(), 0);
        std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return g.send_idx[a] < g.send_idx[b]; });
        std::vector<int32_t> row, ptr;
        for (int64_t i = 0; i < ns; ++i)
            if (i == 0 || g.send_idx[order[i]] != g.send_idx[order[i - 1]]) { row.push_back(g.send_idx[order[i]]); ptr.push_back((int32_t)i); }
        ptr.push_back((int32_t)ns);
        T.n_acc = (int32_t)row.size();
        T.i_acc_row = ix.size(); ix.insert(ix.end(), row.begin(), row.end());
        T.i_acc_ptr = ix.size(); ix.insert(ix.end(), ptr.begin(), ptr.end());
        T.i_acc_pos = ix.size(); ix.insert(ix.end(), order.begin(), order.end());
        const size_t rowb = (size_t)L * 4;
        T.hx_own_b.assign(P, 0); T.hx_own_o.assign(P, 0); T.hx_halo_b.assign(P, 0); T.hx_halo_o.assign(P, 0);
        size_t so = 0, ro = 0;
        for (int q = 0; q < P; ++q) {
            T.hx_own_b[q] = (size_t)g.send_rows[q] * rowb; T.hx_own_o[q] = so; so += T.hx_own_b[q];
            T.hx_halo_b[q] = (size_t)g.recv_rows[q] * rowb; T.hx_halo_o[q] = ro; ro += T.hx_halo_b[q];
        }
        if (so != (size_t)ns * rowb || ro != (size_t)g.n_halo * rowb) return fail(h, MGN_E_STATE, "halo lists and halo counts of the partition disagree");
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, T.idx.ensure(ix.size() * 4));
    HIPCHK(h, hipMemcpy(T.idx.p, ix.data(), ix.size() * 4, hipMemcpyHostToDevice));
    if (part) {
        const size_t ns = g.send_idx.size();
        HIPCHK(h, T.hx_send.ensure(ns * L * 4));
        HIPCHK(h, T.hx_recv.ensure(std::max(ns, (size_t)g.n_halo) * L * 4));
        const size_t stride = (size_t)rank_sum_stride((int64_t)h->params.size()) * 4;
        HIPCHK(h, T.fin_s.ensure(stride));
        HIPCHK(h, T.fin_r.ensure(stride * g.nranks));
        HIPCHK(h, T.fin_loss.ensure(sizeof(double)));
        HIPCHK(h, hipMemset(T.fin_s.p, 0, stride));           // (head and padding stay zero; the gradient is written per call)
    }

    auto layout = [&](int keep) -> size_t {
        size_t off = 0;
        auto take = [&](size_t n) { const size_t o = off; off += (n + 63) / 64 * 64; return o; };
        auto take_acts = [&](size_t n) { Acts a; for (int b = 0; b < NB; ++b) for (int i = 0; i < 3; ++i) a.h[b][i] = take(n); return a; };
        T.nf_raw = take((size_t)NG * h->cfg.Fn);
        T.nf_pad = take(NL);
        T.a_en = take_acts(NL);
        T.a_de = take_acts(NL);
        for (int q = 0; q < S; ++q) {
            T.ef_raw[q] = take((size_t)(part ? g.set[q].E : g.set[q].e_local) * h->es[q].Fe);
            T.ef_pad[q] = take(EL[q]);
            T.a_ee[q] = take_acts(EL[q]);
        }
        // e' = LayerNorm(Y) as an array of its own only where some edge set's forward does not aggregate inside its launch (train.h: SEG_*)
        bool need_enew = h->cfg.ln_dims == MGN_LN_ALL;
        for (int q = 0; q < S; ++q) {
            const int64_t E = g.set[q].e_local;
            need_enew = need_enew || !(E > 0 && train_fwd_fused_agg(L, (int)((E + TILE - 1) / TILE)));
        }
        T.Enew = take(need_enew ? ELmax : 64);
        T.Vk.assign(mps + 1, 0);
        T.Vk[0] = take(NL);
        for (int q = 0; q < S; ++q) {
            T.Ek[q].assign(mps + 1, 0);
            T.agg[q].assign(mps, 0);
            T.a_pe[q].assign(mps, Acts());
            T.Ek[q][0] = take(EL[q]);
        }
        T.a_pn.assign(mps, Acts());
        // Kept activations of the processor: 3 (E + N) L floats per launch unit and step when H1 / H2 / Y are stored.  Small meshes store
        // them all.  Large ones store them for as many steps as the device's free memory holds (the last ones: the reverse pass meets them
        // first) and recompute the rest in the reverse pass (one more forward per MLP; (E + 2 N) L floats per step kept): M-1M needs
        // 61 GB with every step recomputed and 10.7 GB more per stored step, which is worth 4 ms of the step -- the part has 288 GB.
        // The default takes what hipMemGetInfo reports free minus a reserve (MGN_TRAIN_RESERVE_GB, 16): the FIRST handle of a process (or the
        // first process on a device) gets the stored steps, a later one sees what is left and recomputes; the size of the arena with no
        // step stored is taken from a dry run of this very layout, and an allocation that fails all the same (another process took the
        // memory between the query and the request) is retried with fewer stored steps, down to none (train_graph_build's caller).
        // MGN_TRAIN_RECOMPUTE = 0 / 1 forces all / none, MGN_TRAIN_KEEP_STEPS = n the count.
        T.keep_steps = keep;
        T.recompute = T.keep_steps < mps;
        Acts shared_e[MAX_EDGE_SETS], shared_n;
        if (T.recompute) {
            for (int q = 0; q < S; ++q) shared_e[q] = take_acts(EL[q]);
            shared_n = take_acts(NL);
        }
        for (int k = 0; k < mps; ++k) {
            for (int q = 0; q < S; ++q) {
                T.a_pe[q][k] = T.kept(k, mps) ? take_acts(EL[q]) : shared_e[q];
                T.agg[q][k] = take(NL);
                T.Ek[q][k + 1] = take(EL[q]);
            }
            T.a_pn[k] = T.kept(k, mps) ? take_acts(NL) : shared_n;
            T.Vk[k + 1] = take(NL);
        }
        const size_t ML = NL > ELmax ? NL : ELmax;
        // Above the cooperative range the first layer of the edge MLPs is factored as in the inference kernels: per NODE
        // P = v W1_sender, Q = v W1_receiver (2 chunk passes over N rows instead of 2 over E rows), backward and weight gradients
        // through the summed rows of GZ1 (gather <-> segmented-sum duality).  MGN_TRAIN_FACTORED = 0 / 1 overrides the size rule.
        bool any_fact = false, all_fact = true;
        for (int q = 0; q < S; ++q) {
            const int64_t E = g.set[q].e_local;
            T.factored[q] = !train_uses_coop(128, (int)((E + TILE - 1) / TILE));   // the size rule of the cooperative kernels, for every L
            T.factored[q] = env_int("MGN_TRAIN_FACTORED", T.factored[q]) != 0;
            if (E == 0) T.factored[q] = false;
            any_fact = any_fact || T.factored[q];
            all_fact = all_fact && T.factored[q];
        }
        // Small meshes (the cooperative-tile regime: a launch leaves most of the chip idle) get GSETS sets of gradient buffers so
        // that the parameter gradients can run on a second stream; larger ones fill the chip on their own and keep one set.
        {
            const int64_t big = Emax > N ? Emax : N;
            T.gsets = (!part && !T.recompute && !any_fact && L == 128 && big <= (int64_t)TRAIN_COOP_TILES_PER_CU * train_size_cus() * TILE) ? TrainState::GSETS : 1;   // (SGs / SGr are single buffers; a partition runs on one stream, eagerly: communicator calls sit between its launches)
        }
        // GT / G xhat rows only where some LayerNorm'd launch unit does not take its parameter sums inside the backward kernel (train.h: LNSUM)
        bool need_gt = h->cfg.ln_dims == MGN_LN_ALL || T.gsets > 1 || !train_bwd_ln_sums(L, (int)((N + TILE - 1) / TILE));
        for (int q = 0; q < S; ++q) {
            const int64_t E = g.set[q].e_local;
            need_gt = need_gt || (E > 0 && !train_bwd_ln_sums(L, (int)((E + TILE - 1) / TILE)));
        }
        T.need_gt = need_gt;
        for (int i = 0; i < T.gsets; ++i) { T.GT[i] = take(need_gt ? ML : 64); T.GXH[i] = take(need_gt ? ML : 64); T.GY[i] = take(ML); T.GZ2[i] = take(ML); T.GZ1[i] = take(ML); }
        T.GXs = T.GXr = T.Pn = T.Qn = T.SGs = T.SGr = T.GXB = 0;
        if (any_fact) { T.Pn = take(NL); T.Qn = take(NL); T.SGs = take(NL); T.SGr = take(NL); }
        if (!all_fact) { T.GXs = take(ELmax); T.GXr = take(ELmax); }
        if (NB > 1) T.GXB = take(ML);                      // gradient handed from an MLP's second launch unit to its first
        T.gV[0] = take(NL); T.gV[1] = take(NL);
        for (int q = 0; q < S; ++q) { T.gE[q][0] = take(EL[q]); T.gE[q][1] = take(EL[q]); T.gAgg[q] = take(NL); }
        T.Gout = take(NL);
        T.gNF = take(NL);
        T.io = take((size_t)(N > 0 ? N : 1) * (2 * h->cfg.O + h->cfg.Fn + 1));
        T.ptmp = take((size_t)(NG > 0 ? NG : 1) * (size_t)std::max(h->cfg.Fn, h->cfg.O));      // row permutations of a renumbered graph
        int nb = std::max(wgrad_blocks(NT), wgrad_blocks(N));   // the most blocks of any launch unit (the count is not monotonic in the rows once rows per block grow)
        for (int q = 0; q < S; ++q) nb = std::max(nb, wgrad_blocks(g.set[q].e_local));
        T.pw = take((size_t)UNIT_W_JOBS * (nb > 0 ? nb : 1) * L * L);   // one partial-dW region per weight job of a launch, one partial column-sum region per job
        T.pb = take((size_t)WGRAD_MAX_JOBS * (nb > 0 ? nb : 1) * L);
        T.lnsum = take(((ML / L + TILE - 1) / TILE + 7) / 8 * (size_t)2 * L + 2 * L);
        T.lnsum2 = take((size_t)LNSUM_GROUPS * 2 * L);
        T.segcarry = take((size_t)2 * ((ELmax / L + TILE - 1) / TILE + 1) * L);
        if (h->cfg.ln_dims == MGN_LN_ALL) {
            int slot = 0;
            T.m_en.lnslot = slot++;
            for (int q = 0; q < S; ++q) T.m_ee[q].lnslot = slot++;
            for (int k = 0; k < mps; ++k) {
                for (int q = 0; q < S; ++q) T.m_pe[q][k].lnslot = slot++;
                T.m_pn[k].lnslot = slot++;
            }
            T.lnstats = take((size_t)64 * slot);
            const size_t nt_max = (std::max<size_t>(NL, ELmax) / L + TILE - 1) / TILE;
            T.lnpart = take((size_t)2 * std::max<size_t>({(size_t)2 * array_stats_blocks(), (size_t)2 * 128 * lnall_bwd_blocks(), (size_t)2 * 4 * nt_max}));
            T.lnm = take(64);
        }
        return off;
    };
    int keep0 = mps;
    {
        double rows = (double)NL;
        for (int q = 0; q < S; ++q) rows += (double)EL[q];
        const double per_step = 3.0 * NB * rows * 4.0, stored = (double)mps * per_step;
        if (stored > 48e9) {
            keep0 = 0;
            T.arena.release();                             // (an earlier graph's arena must not count as taken)
            size_t free_b = 0, total_b = 0;
            // a companion (mgn_shooting_grad) recomputes: the free memory belongs to its parent's own training arena
            if (!h->companion && hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
                const double reserve = env_double("MGN_TRAIN_RESERVE_GB", 16.0) * 1e9;
                const double base = (double)layout(0) * 4.0;          // the arena with every step recomputed: a dry run of the layout below
                const double room = (double)free_b - base - reserve;
                if (room > 0) keep0 = (int)std::min<double>((double)mps, room / per_step);
            }
        }
        const int recompute = env_int("MGN_TRAIN_RECOMPUTE", INT_MIN);   // unset: by the rule above
        if (recompute != INT_MIN) keep0 = recompute != 0 ? 0 : mps;
        keep0 = std::max(0, std::min(mps, env_int("MGN_TRAIN_KEEP_STEPS", keep0)));
    }
    T.drop_graphs();
    T.traj.ef_pad_ok = false;
    T.batch.ef_ok = false;
    T.size_cus = train_size_cus();
    T.wg_rpb_last = T.wg_rpb_node = 0;
    for (int64_t& v : T.wg_rpb_edge) v = 0;
    size_t off = 0;
    int test_fail = env_int("MGN_TRAIN_TEST_FAIL_ALLOCS", 0);   // n: the first n requests count as refused (tests of the retry)
    for (int keep = keep0;; keep = keep / 2) {            // an allocation that fails is retried with fewer stored steps (none at last)
        off = layout(keep);
        if (test_fail-- <= 0 && T.arena.ensure(off * 4) == hipSuccess) break;
        (void)hipGetLastError();
        T.arena.release();
        if (keep == 0) return fail(h, MGN_E_OOM, "training arena: %.1f GB with every processor step recomputed do not fit the device's free memory", (double)off * 4e-9);
    }
    T.arena_floats = off;
    HIPCHK(h, T.target.ensure((size_t)(N > 0 ? N : 1) * h->cfg.O * 4));
    T.g2l.clear();
    T.mask_valid = false;
    if (h->g.renumbered || part) {      // (-1: a node another rank owns)
        T.g2l.assign((size_t)h->g.N, part ? -1 : 0);
        for (int32_t i = 0; i < h->g.n_own; ++i) T.g2l[(size_t)h->g.own_gid[i]] = i;
    }
    T.graph_ready = true;
    return MGN_OK;
}

}  // namespace
}  // namespace mgn

using namespace mgn;

namespace {

// The five kinds of job that differentiate the model: step! (mgn_step), the pullback of the model call (mgn_forward_vjp), of the right-hand
// side (mgn_ode_vjp), one step of a reverse sweep (mgn_solver_grad and its kin: the right-hand side's, on resident inputs), and step! on
// one datapoint of the resident trajectory (mgn_step_datapoint: init_train_step on the device, then mgn_step's stages).  JOB_DATAPOINTS
// is step! on B datapoints at once (mgn_step_datapoints): it runs on the companion of B copies, its inputs come from the parent handle
enum JobKind { JOB_STEP, JOB_FORWARD_VJP, JOB_RHS_VJP, JOB_SWEEP_STEP, JOB_DATAPOINT, JOB_DATAPOINTS };

struct TrainJob {
    JobKind kind = JOB_STEP;
    // step!: the FeatureGraph as given, target, mask
    const float* nf = nullptr; const float* ef = nullptr; const float* target = nullptr;
    const int32_t* mask = nullptr; int64_t nmask = 0; int32_t mask_index_base = 0;
    float* loss = nullptr;
    // vjp of the RHS: raw inputs of mgn_ode_step (ef = raw edge features), cotangent lambda
    const float* x = nullptr; const float* onehot = nullptr; const float* val_mask = nullptr; const float* lambda = nullptr;
    float* dxdt = nullptr; float* xbar = nullptr;
    float* grads = nullptr;
    // vjp of the model itself (mgn_forward_vjp): nf / ef as in step!, cotangent `lambda` of the output, gradient of all of nf out
    float* nfbar = nullptr; float* out = nullptr;
    // one step of the reverse sweep of mgn_solver_grad: x is a device slot in the engine's order, lambda is already in its io slot
    // and the statics in theirs (Sweep::begin staged them); xbar stays in io, the gradient is added to gacc (first: gacc = it), no synchronisation
    bool first = false;
    double* gacc = nullptr;
    // step! on a datapoint of the resident trajectory (TrainState::traj): mask, loss and grads as for step!
    int32_t datapoint = 0; bool accumulate = false;
    // step! on B datapoints of the PARENT's resident trajectory (the job's own handle is the companion of B copies): mask (listed once,
    // the parent's node ids), loss (the mean) and grads as for step!, losses [B] (null: not wanted)
    mgn_engine* parent = nullptr; const int32_t* datapoints = nullptr; int32_t B = 0; float* losses = nullptr;
};

// partitions: the entry point runs on a partitioned mesh (mgn_step); every check comes before the first collective
int train_prepare(mgn_handle* h, const char* who, size_t n_grads, bool partitions = false) {
    if (int rc = width_refuse(h, who)) return rc;
    if (int rc = need(h, true, true, false, true)) return rc;    // (the training kernels pack their own weights from h->params)
    const mgn_config& c = h->cfg;
    if (c.nranks != 1 && !partitions) return fail(h, MGN_E_STATE, "%s drives one partition", who);
    if (c.nranks != 1 && h->nsets != 1) return fail(h, MGN_E_UNSUPPORTED, "%s on a partitioned mesh takes one edge set", who);
    if (c.nranks != 1 && !h->comm)
        return fail(h, MGN_E_STATE, "%s with nranks = %d needs a communicator: call mgn_comm_init on every rank first", who, c.nranks);
    if (c.dtype != MGN_F32) return fail(h, MGN_E_STATE, "%s computes in fp32: create the handle with dtype MGN_F32", who);
    for (int q = 1; q < h->nsets; ++q)
        if (h->g.set[q].E > 0 && !h->es[q].have_ef)
            return fail(h, MGN_E_STATE, "edge set %d has edges but no features: call mgn_set_edge_features after mgn_set_edge_set", q);
    if (n_grads != h->params.size()) return fail(h, MGN_E_ARG, "%s: grads has %zu floats, model has %zu", who, n_grads, h->params.size());
    if (!h->train) h->train = new (std::nothrow) TrainState();
    if (!h->train) return fail(h, MGN_E_OOM, "host allocation failed");
    if (!h->train->packed)
        if (int rc = pack_training_weights(h)) return rc;
    if (!h->train->graph_ready || h->train->size_cus != train_size_cus())   // (the arena's placeholders follow the size rules the launches read)
        if (int rc = prepare_graph(h)) return rc;
    return MGN_OK;
}

// ---- mgn_step_datapoint: one datapoint's nf_pad, target and ef_pad from the resident trajectory (TrainState::traj) ----
int online_dim(const mgn_config& c, int g) { return g == 1 ? c.Fe : c.O; }
size_t online_off(const mgn_config& c, int g) { return g == 0 ? 0 : (g == 1 ? (size_t)2 * c.O : (size_t)2 * c.O + 2 * c.Fe); }
int online_totals_ready(mgn_engine* h) {
    DevBuf& b = h->train->on_totals;
    if (b.p) return MGN_OK;
    const size_t bytes = (size_t)(4 * h->cfg.O + 2 * h->cfg.Fe) * sizeof(double);
    HIPCHK(h, b.ensure(bytes));
    HIPCHK(h, hipMemsetAsync(b.p, 0, bytes, h->stream));
    return MGN_OK;
}
// h->norms exists (identity maps where mgn_set_norms was never called) and an online group's map is applied
int datapoint_norms_ready(mgn_engine* h) {
    const mgn_config& c = h->cfg;
    const size_t n = (size_t)2 * (c.Fn + c.Fe + c.O);
    if (!h->norms.p || h->norms.bytes < n * 4) {
        std::vector<float> v(n, 0.f);
        float* q = v.data();
        for (int d : {c.Fn, c.Fe, c.O}) {
            for (int i = 0; i < d; ++i) q[i] = 1.f;
            q += 2 * d;
        }
        HIPCHK(h, hipStreamSynchronize(h->stream));
        HIPCHK(h, h->norms.ensure(n * 4));
        HIPCHK(h, hipMemcpy(h->norms.p, v.data(), n * 4, hipMemcpyHostToDevice));
        h->norms_host = v;
        h->norms_host_stale = false;
    }
    const TrainState& T = *h->train;
    if (T.on[0].online) h->have_nnorm = true;
    if (T.on[1].online) h->have_enorm = true;
    if (T.on[2].online) h->have_onorm = true;
    return MGN_OK;
}
DatapointArgs datapoint_args(mgn_engine* h, int32_t t, bool normalised) {
    const TrainState::Trajectory& R = h->train->traj;
    const mgn_config& c = h->cfg;
    const int64_t N = h->g.n_own;
    const float* nrm = h->norms.as<float>();
    DatapointArgs a{};
    a.cur = R.frames.as<float>() + (size_t)t * (size_t)N * c.O;       // (64-bit: T N O passes 2^31 on the largest meshes)
    a.nxt = a.cur + (size_t)N * c.O;
    a.onehot = c.Fn > c.O ? R.onehot.as<float>() : nullptr;
    a.gid = h->g.renumbered || c.nranks > 1 ? h->d_own_gid.as<int32_t>() : nullptr;   // (a partition's rows are the nodes it owns)
    a.noisy = R.noise && R.some_nodes ? R.noisy.as<uint8_t>() : nullptr;
    a.stddev = R.noise ? R.stddev.as<float>() : nullptr;
    a.nrm_n = normalised && h->have_nnorm ? nrm : nullptr;
    a.nrm_o = normalised && h->have_onorm ? nrm + 2 * c.Fn + 2 * c.Fe : nullptr;
    a.N = N; a.O = c.O; a.Fn = c.Fn; a.ld = c.Fn; a.t = t;
    a.Nkey = c.nranks > 1 ? h->g.N : N;               // the noise is keyed by the caller's node id among all nodes of the mesh
    a.delta = R.delta[(size_t)t];
    a.seed = R.seed;
    return a;
}
// The normaliser call of the reference accumulates, then normalises: an accumulating step adds the datapoint's raw rows (cur, ef_raw, d)
// to the totals of every online group that still accumulates and rewrites that group's entries of h->norms, all on the device; restored
// totals (mgn_train_norm_state) get their maps here as well.  No copy to the host, no synchronisation; count and calls are host numbers.
// A partition (nranks > 1) forms the sums of the rows it owns -- every node and every edge lives on exactly one rank --, folds its
// block partials in block order, and one allgather on the handle's stream brings every rank's sums to every rank; they are added to
// the totals in ascending rank order, so totals and maps are the same bits on all ranks.  Whether a group accumulates is decided
// from the mesh's counts and from host state that all ranks share, never from what this rank owns: every rank joins every allgather.
int datapoint_norms(mgn_engine* h, int32_t t, bool accumulate, hipStream_t st) {
    if (int rc = datapoint_norms_ready(h)) return rc;
    TrainState& T = *h->train;
    TrainState::Trajectory& R = T.traj;
    const mgn_config& c = h->cfg;
    const bool multi = c.nranks > 1;
    const int P = c.nranks;
    const int64_t N = h->g.n_own, E = h->g.set[0].e_local;
    const int64_t NG = multi ? h->g.N : N, EG = multi ? h->g.set[0].E : E;    // rows of the whole mesh
    // this rank's sums and all ranks' (doubles): [cur sum, sum of squares | d ...] = 4 O per rank, then the edge features' 2 Fe per rank
    const size_t xs_n = (size_t)4 * c.O, xs_e = (size_t)2 * c.Fe;
    auto comm_fail = [&](const char* what) { return fail(h, MGN_E_RCCL, "mgn_step_datapoint: %s: %s", what, h->comm->err.c_str()); };
    bool add[3], write[3], any = false;
    for (int g = 0; g < 3; ++g) {
        const int64_t rows = g == 1 ? EG : NG;
        add[g] = accumulate && T.on[g].online && T.on[g].calls < T.on[g].max_acc && rows > 0;
        write[g] = T.on[g].online && (add[g] || T.on[g].dirty);
        any = any || write[g];
    }
    if (!any) return MGN_OK;
    if (int rc = online_totals_ready(h)) return rc;
    if (multi && !R.xsum.p) HIPCHK(h, R.xsum.ensure((size_t)(P + 1) * (xs_n + xs_e) * sizeof(double)));
    double* const xs = multi ? R.xsum.as<double>() : nullptr;
    double* const xs_all_n = multi ? xs + xs_n + xs_e : nullptr;
    double* const xs_all_e = multi ? xs_all_n + (size_t)P * xs_n : nullptr;
    int nb = stats_blocks(N);
    int pstride = 0;
    const double *p0 = nullptr, *p2 = nullptr;
    if (add[0] || add[2]) {
        const size_t rawf = ((size_t)N * c.O + 63) / 64 * 64, partd = (size_t)nb * 2 * c.O;
        HIPCHK(h, R.work.ensure(2 * rawf * 4 + 2 * partd * sizeof(double)));
        float* rcur = R.work.as<float>();
        float* rd = rcur + rawf;
        double* part = reinterpret_cast<double*>(rd + rawf);
        DatapointArgs a = datapoint_args(h, t, false);
        a.ld = c.O; a.raw_cur = rcur; a.raw_d = rd; a.raw_local = multi ? 1 : 0;
        HIPCHK(h, launch_datapoint_assemble(a, st));
        if (add[0]) { HIPCHK(h, launch_col_stats(rcur, N, c.O, part, st)); p0 = part; }
        if (add[2]) { HIPCHK(h, launch_col_stats(rd, N, c.O, part + partd, st)); p2 = part + partd; }
        if (multi) {                   // the owned rows' sums, folded in block order; then all ranks' sums, which the totals take in rank order
            HIPCHK(h, hipMemsetAsync(xs, 0, xs_n * sizeof(double), st));
            NormsFromTotalsArgs z{};
            if (add[0]) { z.g[0].partial = p0; z.g[0].totals = xs; z.g[0].nb = nb; z.g[0].dim = c.O; z.g[0].add = 1; }
            if (add[2]) { z.g[2].partial = p2; z.g[2].totals = xs + 2 * c.O; z.g[2].nb = nb; z.g[2].dim = c.O; z.g[2].add = 1; }
            HIPCHK(h, launch_norms_from_totals(z, st));
            if (h->comm->allgather(xs, xs_n * sizeof(double), xs_all_n, st) != 0) return comm_fail("allgather of the normalisers' sums");
            p0 = xs_all_n; p2 = xs_all_n + 2 * c.O;
            nb = P; pstride = (int)xs_n;
        }
    }
    if (add[1] && !R.ef_sums_ok) {     // what one accumulation of ef_raw adds: the same terms in the same order, formed once per trajectory
        const int nbe = stats_blocks(E);
        const size_t head = (size_t)2 * c.Fe * sizeof(double);
        HIPCHK(h, R.ef_sums.ensure(head + (size_t)nbe * head));
        double* sums = R.ef_sums.as<double>();
        double* own = multi ? xs + xs_n : sums;            // (a partition: its local edges' sums first, the mesh's from all ranks' below)
        HIPCHK(h, hipMemsetAsync(own, 0, head, st));
        HIPCHK(h, launch_col_stats(R.ef_raw.as<float>(), E, c.Fe, sums + 2 * c.Fe, st));
        NormsFromTotalsArgs z{};
        z.g[0].partial = sums + 2 * c.Fe; z.g[0].totals = own; z.g[0].nb = nbe; z.g[0].dim = c.Fe; z.g[0].add = 1;
        HIPCHK(h, launch_norms_from_totals(z, st));
        if (multi) {                   // (a rank without an edge sends zeros)
            if (h->comm->allgather(own, head, xs_all_e, st) != 0) return comm_fail("allgather of the edge features' sums");
            HIPCHK(h, hipMemsetAsync(sums, 0, head, st));
            NormsFromTotalsArgs y{};
            y.g[0].partial = xs_all_e; y.g[0].totals = sums; y.g[0].nb = P; y.g[0].dim = c.Fe; y.g[0].add = 1;
            HIPCHK(h, launch_norms_from_totals(y, st));
        }
        R.ef_sums_ok = true;
    }
    float* nrm = h->norms.as<float>();
    float* scale[3] = {nrm, nrm + 2 * c.Fn, nrm + 2 * c.Fn + 2 * c.Fe};
    const int stride[3] = {c.Fn, c.Fe, c.O};
    NormsFromTotalsArgs a{};
    for (int g = 0; g < 3; ++g) {
        if (!write[g]) continue;
        TrainState::OnlineGroup& o = T.on[g];
        if (add[g]) { o.count += (double)(g == 1 ? EG : NG); o.calls += 1.0; }
        NormGroupArgs& q = a.g[g];
        q.partial = g == 0 ? p0 : (g == 2 ? p2 : nullptr);
        q.call_sums = g == 1 ? R.ef_sums.as<double>() : nullptr;
        q.totals = T.on_totals.as<double>() + online_off(c, g);
        q.scale = scale[g]; q.shift = scale[g] + stride[g];
        q.count = o.count; q.eps = o.eps; q.nb = nb; q.pstride = pstride; q.dim = online_dim(c, g);
        q.add = add[g] ? 1 : 0; q.write = 1; q.inverse = g == 2 ? 1 : 0;
        o.dirty = false;
    }
    HIPCHK(h, launch_norms_from_totals(a, st));
    h->norms_host_stale = true;        // (its two readers refresh it: sync_norms_host)
    invalidate_static(h);              // as mgn_set_norms does
    if (write[1]) { R.ef_pad_ok = false; ++R.ef_gen; }
    return MGN_OK;
}
int datapoint_stage(mgn_engine* h, int32_t t, bool accumulate, hipStream_t st) {
    if (int rc = datapoint_norms(h, t, accumulate, st)) return rc;
    TrainState& T = *h->train;
    TrainState::Trajectory& R = T.traj;
    const mgn_config& c = h->cfg;
    float* A = T.arena.as<float>();
    DatapointArgs a = datapoint_args(h, t, true);
    a.nf = A + T.nf_pad; a.ld = c.L; a.target = T.target.as<float>();
    HIPCHK(h, launch_datapoint_assemble(a, st));
    const int64_t E = h->g.set[0].e_local;
    if (!R.ef_pad_ok && E > 0) {       // a constant of the trajectory: rebuilt when the trajectory, the norms or the arena changed
        const float* es = h->have_enorm ? h->norms.as<float>() + 2 * c.Fn : nullptr;
        HIPCHK(h, launch_affine_pad(R.ef_raw.as<float>(), c.Fe, nullptr, 0, es, es ? es + c.Fe : nullptr, A + T.ef_pad[0], c.L, E, st));
    }
    R.ef_pad_ok = true;
    return MGN_OK;
}
// mgn_step_datapoints: nf_pad, target and (when stale) ef_pad of the companion c's arena from the parent h's resident trajectory, under
// h's device norms as they stand after the call's accumulations -- accumulate first, normalise afterwards: the B datapoints' raw rows go
// into the totals one datapoint at a time in the order listed, each as one call of datapoint_norms (its reduction, its order, count and
// calls per datapoint), then one launch assembles all B under the resulting maps.  No copy of the norms, no synchronisation.
int datapoints_stage(mgn_engine* h, mgn_engine* c, const int32_t* ts, int32_t B, bool accumulate, hipStream_t st) {
    if (accumulate) {
        for (int32_t b = 0; b < B; ++b)
            if (int rc = datapoint_norms(h, ts[b], true, st)) return rc;
    } else if (int rc = datapoint_norms(h, ts[0], false, st)) {    // (restored totals get their maps here)
        return rc;
    }
    const TrainState::Trajectory& R = h->train->traj;
    TrainState& T = *c->train;
    const mgn_config& k = h->cfg;
    const int64_t N = h->g.n_own, E = h->g.set[0].e_local;
    float* A = T.arena.as<float>();
    const float* nrm = h->norms.as<float>();
    DatapointBatchArgs a{};
    a.frames = R.frames.as<float>();
    a.onehot = k.Fn > k.O ? R.onehot.as<float>() : nullptr;
    a.gid = h->g.renumbered ? h->d_own_gid.as<int32_t>() : nullptr;
    a.noisy = R.noise && R.some_nodes ? R.noisy.as<uint8_t>() : nullptr;
    a.stddev = R.noise ? R.stddev.as<float>() : nullptr;
    a.nrm_n = h->have_nnorm ? nrm : nullptr;
    a.nrm_o = h->have_onorm ? nrm + 2 * k.Fn + 2 * k.Fe : nullptr;
    a.nf = A + T.nf_pad; a.target = T.target.as<float>();
    a.N = N; a.B = B; a.O = k.O; a.Fn = k.Fn; a.ld = k.L;
    a.seed = R.seed;
    for (int32_t b = 0; b < B; ++b) { a.t[b] = ts[b]; a.delta[b] = R.delta[(size_t)ts[b]]; }
    HIPCHK(h, launch_datapoints_assemble(a, st));
    if (E > 0 && (!T.batch.ef_ok || T.batch.ef_gen != R.ef_gen)) {   // a constant of the trajectory: rebuilt when the trajectory, the norms or the companion's arena changed
        const float* es = h->have_enorm ? nrm + 2 * k.Fn : nullptr;
        HIPCHK(h, launch_datapoints_edges(R.ef_raw.as<float>(), k.Fe, es, es ? es + k.Fe : nullptr, h->es[0].d_edge_gid.as<int64_t>(), A + T.ef_pad[0], k.L, E, B, st));
    }
    T.batch.ef_ok = true;
    T.batch.ef_gen = R.ef_gen;
    return MGN_OK;
}
// what every entry point of the datapoint family asks of the handle before it looks at its arguments
int datapoint_need(mgn_handle* h, const char* who, bool graph, bool trajectory) {
    if (int rc = width_refuse(h, who)) return rc;
    if (int rc = need(h, false, graph)) return rc;
    if (h->cfg.nranks != 1 && h->nsets != 1) return fail(h, MGN_E_UNSUPPORTED, "%s on a partitioned mesh takes one edge set", who);
    if (h->cfg.nranks != 1 && !h->comm)
        return fail(h, MGN_E_STATE, "%s with nranks = %d needs a communicator: call mgn_comm_init on every rank first", who, h->cfg.nranks);
    if (h->cfg.dtype != MGN_F32) return fail(h, MGN_E_STATE, "%s computes in fp32: create the handle with dtype MGN_F32", who);
    if (trajectory && (!h->train || !h->train->traj.have))
        return fail(h, MGN_E_STATE, "%s: no trajectory: call mgn_train_set_trajectory after mgn_set_graph (a new graph drops it)", who);
    if (!h->train) h->train = new (std::nothrow) TrainState();
    if (!h->train) return fail(h, MGN_E_OOM, "host allocation failed");
    return MGN_OK;
}

// The first launch unit's inputs of an MLP forward: rows / ntiles and up to three blocks of rows, gathered where an index is given
TrainFwdArgs fwd_inputs(int64_t rows, int32_t ntiles, const float* x0, const int32_t* i0 = nullptr, const float* x1 = nullptr,
                        const int32_t* i1 = nullptr, const float* x2 = nullptr) {
    TrainFwdArgs a{};
    a.rows = rows; a.ntiles = ntiles;
    a.X[0] = x0; a.xidx[0] = i0; a.X[1] = x1; a.xidx[1] = i1; a.X[2] = x2;
    return a;
}
// One MLP forward = one or two launch units (TrainPass::run_fwd, LnAll::mlp).  What unit bi's launch takes from the MLP itself: `in` carries
// rows / ntiles and the first unit's inputs (X, xidx, PRE, preidx); w1sel >= 0: only block w1sel of W1 is applied per row (the factored
// edge MLP: the e block); the second unit reads the first one's output `chained` (its Y: no LayerNorm, no residual).  Where the
// activations and the output go is the caller's.  Returns the launch's layer-1 input blocks.
int fwd_unit(const TrainMlp& m, int bi, const TrainFwdArgs& in, int w1sel, const float* Wt, const float* chained, TrainFwdArgs& a) {
    const TrainBlock& b = m.b[bi];
    a = TrainFwdArgs{};
    a.rows = in.rows; a.ntiles = in.ntiles;
    a.W2 = Wt + b.W2; a.W3 = Wt + b.W3; a.tabs = Wt + b.tabs;
    if (bi > 0) {
        a.X[0] = chained;
        a.W1[0] = Wt + b.W1[0];
        return b.nin;
    }
    for (int j = 0; j < 3; ++j) { a.X[j] = in.X[j]; a.xidx[j] = in.xidx[j]; }
    for (int j = 0; j < 2; ++j) { a.PRE[j] = in.PRE[j]; a.preidx[j] = in.preidx[j]; }
    if (w1sel >= 0) { a.W1[0] = Wt + b.W1[w1sel]; return 1; }
    for (int j = 0; j < b.nin; ++j) a.W1[j] = Wt + b.W1[j];
    return b.nin;
}

// What the backward of one launch unit reads and leaves besides its block and its kept activations: the upstream gradient g0[row]
// (+ g1[g1i[row]]); per layer-1 input block j the gradient gx[j] = (gxadd[j]) + GZ1 W1T[j] (null: not wanted) and the input xin[j], gathered by
// xi[j], that the block's weight gradient takes.
// fq >= 0: first unit of the edge MLP of set fq with the factored first layer -- only the e block of W1 is unwound per edge
// (gx[0] / gxadd[0] / xin[0] describe it); the v blocks follow per node from the summed rows of GZ1 (SGs, SGr) and the node latents vin.
struct BwdIo {
    const float* g0 = nullptr; const float* g1 = nullptr; const int32_t* g1i = nullptr;
    float* gx[3] = {}; const float* gxadd[3] = {};
    const float* xin[3] = {}; const int32_t* xi[3] = {};
    int fq = -1; const float* vin = nullptr;
};

// one launch unit as its weight-gradient launch sees it, after its activation backward has been issued into gradient-buffer set gs
struct WgradUnit {
    const TrainBlock& b; const BwdIo& io;
    const size_t* hb;            // its kept H1, H2, Y
    int64_t rows, node_rows; int32_t ntiles; int gs;
    bool wide, lnsum;            // how its LayerNorm parameters get their sums (TrainPass::bwd_unit)
};

// One pass of the model and its pullback over the training arena: forward with kept activations, seed, reverse pass, all parameter
// gradients (+ the input gradient for the VJPs).  Built per call from the handle and the job; train_run below is the sequence of its stages.
struct TrainPass {
    struct SetIdx { int64_t E; int32_t nt; const int32_t *egid, *perm_s, *rowptr_s, *snd, *rcv, *rowptr; };
    mgn_engine* h;
    const TrainJob& J;
    const mgn_config& c;
    TrainState& T;
    const LocalGraph& g;
    const int S, L, mps, O;
    // a partition (train_prepare with `partitions`: mgn_step, the datapoint step, and through the group the VJPs and the sweeps; one edge set): N owned rows, then the halo rows; the caller's arrays are the whole mesh's
    const bool part;
    const int64_t N, NT, NG;
    const int32_t nt_n, nt_t;
    hipStream_t st;
    float* A;
    const float* Wt;
    SetIdx sx[MAX_EDGE_SETS] = {};
    float* G;                    // the gradient of this pass (a partition's is its term of the finish)
    const float* nrm;            // [node scale, shift (Fn) | edge scale, shift (Fe) | out scale, shift (O)]
    // A renumbered graph (graph_host.h: the engine's node order is not the caller's): per-node inputs are brought into the engine's
    // order as they arrive and per-node results go back through the inverse; `mask` is mapped on the host.  Edges go by edge_gid already.
    const bool renum;            // (a partition's rows are the rows it owns, wherever they lie in the caller's arrays)
    const int32_t* ngid;
    const int32_t *acc_row, *acc_ptr, *acc_pos;   // the owners' side of the reverse halo exchange (prepare_graph)
    // ln_dims = MGN_LN_ALL: every LayerNorm takes its statistics over the whole rows x L output of its MLP: the MLP
    // kernels run without their row-wise LayerNorm; two reductions and an elementwise pass follow them in both directions
    const bool lnall;
    const float ln_eps_in, ln_eps_out;
    const bool overlap;          // weight gradients on the second stream (wgrad_unit)
    int64_t lrows_all;           // the longest job of the model: what a launch on the second stream is sized for
    int nlb = 0;                 // partial sums of the loss (seed -> results)
    int n_bwd = 0;               // activation backwards issued in this reverse pass

    TrainPass(mgn_engine* h_, const TrainJob& J_)
        : h(h_), J(J_), c(h_->cfg), T(*h_->train), g(h_->g), S(h_->nsets), L(c.L), mps(c.mps), O(c.O), part(c.nranks > 1), N(g.n_own),
          NT(N + g.n_halo), NG(part ? g.N : N), nt_n((int32_t)((N + TILE - 1) / TILE)), nt_t((int32_t)((NT + TILE - 1) / TILE)), st(h_->stream),
          A(T.arena.as<float>()), Wt(T.w.as<float>()), G(part ? T.fin_s.as<float>() + RANK_SUM_HEAD : T.grads.as<float>()),
          nrm(h_->norms.as<float>()), renum(g.renumbered || part), ngid(h_->d_own_gid.as<int32_t>()),
          acc_row(T.idx.as<int32_t>() + T.i_acc_row), acc_ptr(T.idx.as<int32_t>() + T.i_acc_ptr), acc_pos(T.idx.as<int32_t>() + T.i_acc_pos),
          lnall(c.ln_dims == MGN_LN_ALL), ln_eps_in(c.ln_mode == MGN_LN_STD_EPS ? 0.f : 1e-5f), ln_eps_out(c.ln_mode == MGN_LN_STD_EPS ? 1e-5f : 0.f),
          overlap(T.gsets > 1), lrows_all(N) {
        for (int q = 0; q < S; ++q) {
            sx[q].E = g.set[q].e_local;
            sx[q].nt = (int32_t)((sx[q].E + TILE - 1) / TILE);
            sx[q].egid = T.idx.as<int32_t>() + T.i_egid[q];
            sx[q].perm_s = T.idx.as<int32_t>() + T.i_perm[q];
            sx[q].rowptr_s = T.idx.as<int32_t>() + T.i_rowptr_s[q];
            sx[q].snd = h->es[q].d_snd.as<int32_t>();
            sx[q].rcv = h->es[q].d_rcv.as<int32_t>();
            sx[q].rowptr = h->es[q].d_rowptr.as<int32_t>();
            lrows_all = std::max<int64_t>(lrows_all, sx[q].E);
        }
    }
    bool vjp() const { return J.kind != JOB_STEP && J.kind != JOB_DATAPOINT && J.kind != JOB_DATAPOINTS; }
    float* io() const { return A + T.io; }    // the VJPs' rows: x [N][O] | lambda [N][O] | onehot [N][Fn-O] | val_mask [N]
    int comm_fail(const char* what) { return fail(h, MGN_E_RCCL, "mgn_step: %s: %s", what, h->comm->err.c_str()); }

    // ---- inputs
    hipError_t permute(float* buf, int width, bool inverse) {
        if (!renum || width <= 0) return hipSuccess;
        if (hipError_t e = launch_permute_rows(A + T.ptmp, buf, ngid, N, width, inverse, st)) return e;
        return hipMemcpyAsync(buf, A + T.ptmp, (size_t)N * width * 4, hipMemcpyDeviceToDevice, st);
    }
    hipError_t to_local(float* buf, int width) { return permute(buf, width, false); }    // buf [N][width]: caller's order -> engine's, in place
    hipError_t to_global(float* buf, int width) { return permute(buf, width, true); }    // ... and back
    // An array the caller keeps on the device is read where it is; a host array is staged first.  Gather (renumbered graph) and padding
    // run in the one kernel that reads it (as copy + permute + copy back + pad the eager prologue of a step was 14 launches, 0.24 ms on
    // the cylinder mesh).
    static bool on_device(const void* ptr) {
        hipPointerAttribute_t at{};
        const bool dev = ptr && hipPointerGetAttributes(&at, ptr) == hipSuccess && (at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged);
        (void)hipGetLastError();
        return dev;
    }
    hipError_t staged(const float* user, float* stage, size_t floats, const float*& out) {
        if (on_device(user)) { out = user; return hipSuccess; }
        out = stage;
        return hipMemcpyAsync(stage, user, floats * 4, hipMemcpyHostToDevice, st);
    }
    // step! and the model's VJP: the FeatureGraph's node and edge features as given
    int stage_features() {
        const float* src = nullptr;
        T.traj.ef_pad_ok = false;
        T.batch.ef_ok = false;             // (a companion's arena: mgn_shooting_grad's sweep writes its own edge rows here)
        HIPCHK(h, staged(J.nf, A + T.nf_raw, (size_t)NG * c.Fn, src));
        HIPCHK(h, launch_affine_pad_gather(src, c.Fn, nullptr, 0, nullptr, nullptr, renum ? ngid : nullptr, A + T.nf_pad, L, N, st));
        if (part && g.set[0].E > 0) {      // the local edges' rows of the global array, in the engine's order
            HIPCHK(h, staged(J.ef, A + T.ef_raw[0], (size_t)g.set[0].E * c.Fe, src));
            HIPCHK(h, launch_affine_pad_gather(src, c.Fe, nullptr, 0, nullptr, nullptr, sx[0].egid, A + T.ef_pad[0], L, sx[0].E, st));
        } else if (sx[0].E > 0) {
            HIPCHK(h, staged(J.ef, A + T.ef_raw[0], (size_t)sx[0].E * c.Fe, src));
            HIPCHK(h, launch_affine_pad(src, c.Fe, nullptr, 0, nullptr, nullptr, A + T.ef_pad[0], L, sx[0].E, st));
        }
        return MGN_OK;
    }
    int stage_step() {
        if (int rc = stage_features()) return rc;
        if (renum) {
            const float* src = nullptr;
            HIPCHK(h, staged(J.target, A + T.ptmp, (size_t)NG * O, src));
            HIPCHK(h, launch_permute_rows(T.target.as<float>(), src, ngid, N, O, false, st));
        } else {
            HIPCHK(h, hipMemcpyAsync(T.target.p, J.target, (size_t)N * O * 4, hipMemcpyDefault, st));
        }
        return stage_mask();
    }
    int stage_mask() { return stage_mask_by(renum, T.g2l); }
    // map: the mask lists the caller's node ids of a renumbered graph (or of a partition), g2l takes them to engine rows
    int stage_mask_by(bool map, const std::vector<int32_t>& g2l) {
        // the mask of the previous call is usually this call's (one trajectory, one mask: reference src/MeshGraphNets.jl:352): uploaded once
        const bool mask_dev = on_device(J.mask);
        const bool same = !mask_dev && T.mask_valid && T.mask_base == J.mask_index_base && (int64_t)T.mask_seen.size() == J.nmask &&
                          (J.nmask == 0 || memcmp(T.mask_seen.data(), J.mask, (size_t)J.nmask * 4) == 0);
        if (same) return MGN_OK;
        HIPCHK(h, T.mask.ensure((size_t)J.nmask * 4));
        T.mask_valid = false;
        if (map) {                         // the caller's node ids -> engine rows (0-based from here on)
            std::vector<int32_t> host_mask;
            const int32_t* mk = J.mask;
            if (mask_dev) {
                host_mask.resize((size_t)J.nmask);
                HIPCHK(h, hipMemcpy(host_mask.data(), J.mask, (size_t)J.nmask * 4, hipMemcpyDeviceToHost));
                mk = host_mask.data();
            }
            T.mask_host.clear();
            for (int64_t i = 0; i < J.nmask; ++i) {
                const int32_t l = g2l[(size_t)(mk[i] - J.mask_index_base)];
                if (l >= 0) T.mask_host.push_back(l);       // (a partition takes the entries it owns, as often as they are listed)
            }
            T.mask_n = (int64_t)T.mask_host.size();
            HIPCHK(h, hipMemcpyAsync(T.mask.p, T.mask_host.data(), (size_t)T.mask_n * 4, hipMemcpyHostToDevice, st));
        } else {
            T.mask_n = J.nmask;
            HIPCHK(h, hipMemcpyAsync(T.mask.p, J.mask, (size_t)J.nmask * 4, hipMemcpyDefault, st));
        }
        if (!mask_dev) {
            T.mask_seen.assign(J.mask, J.mask + J.nmask);
            T.mask_base = J.mask_index_base;
            T.mask_valid = true;
        }
        return MGN_OK;
    }
    // A per-node input [rows of the caller's array][width] of a VJP into dst [N][width] in the engine's order.  One partition: copied and
    // permuted in place as ever; a partition takes the rows it owns out of the whole mesh's array (staged in ptmp when it is on the host)
    int stage_rows(const float* user, int width, float* dst) {
        if (!part) {
            HIPCHK(h, hipMemcpyAsync(dst, user, (size_t)N * width * 4, hipMemcpyDefault, st));
            HIPCHK(h, to_local(dst, width));
            return MGN_OK;
        }
        const float* src = nullptr;
        HIPCHK(h, staged(user, A + T.ptmp, (size_t)NG * width, src));
        HIPCHK(h, launch_permute_rows(dst, src, ngid, N, width, false, st));
        return MGN_OK;
    }
    int stage_forward_vjp() {
        if (int rc = stage_features()) return rc;
        return stage_rows(J.lambda, O, io() + (size_t)N * O);
    }
    // RHS inputs exactly as mgn_ode_step takes them: nf = [n_norm(x); n_norm(onehot)], ef = e_norm(ef_raw).
    // The padded node features from a state x [N][O] in the engine's order and the one-hot rows in io
    int pad_state(const float* x) {
        HIPCHK(h, launch_affine_pad(x, O, io() + (size_t)2 * N * O, c.Fn - O, h->have_nnorm ? nrm : nullptr, h->have_nnorm ? nrm + c.Fn : nullptr,
                                    A + T.nf_pad, L, N, st));
        return MGN_OK;
    }
    // The statics of a right-hand side -- one-hot node types and val_mask into io, the normalised raw edge features into ef_pad -- per call of
    // mgn_ode_vjp, once per sweep (Sweep::begin: no state yet, x = null); the state's padding sits between them as the launches always ran
    int stage_statics(const float* x) {
        if (c.Fn > O)
            if (int rc = stage_rows(J.onehot, c.Fn - O, io() + (size_t)2 * N * O)) return rc;
        if (J.val_mask)
            if (int rc = stage_rows(J.val_mask, 1, io() + (size_t)N * (O + c.Fn))) return rc;
        if (x) if (int rc = pad_state(x)) return rc;
        T.traj.ef_pad_ok = false;
        T.batch.ef_ok = false;             // (a companion's arena: mgn_shooting_grad's sweep writes its own edge rows here)
        if (part && g.set[0].E > 0) {      // the local edges' rows of the whole mesh's array, in the engine's order (as stage_features)
            const float* src = nullptr;
            HIPCHK(h, staged(J.ef, A + T.ef_raw[0], (size_t)g.set[0].E * c.Fe, src));
            HIPCHK(h, launch_affine_pad_gather(src, c.Fe, nullptr, 0, h->have_enorm ? nrm + 2 * c.Fn : nullptr,
                                               h->have_enorm ? nrm + 2 * c.Fn + c.Fe : nullptr, sx[0].egid, A + T.ef_pad[0], L, sx[0].E, st));
        } else if (sx[0].E > 0) {
            HIPCHK(h, hipMemcpyAsync(A + T.ef_raw[0], J.ef, (size_t)sx[0].E * c.Fe * 4, hipMemcpyDefault, st));
            HIPCHK(h, launch_affine_pad(A + T.ef_raw[0], c.Fe, nullptr, 0, h->have_enorm ? nrm + 2 * c.Fn : nullptr,
                                        h->have_enorm ? nrm + 2 * c.Fn + c.Fe : nullptr, A + T.ef_pad[0], L, sx[0].E, st));
        }
        return MGN_OK;
    }
    int stage_rhs_vjp() {
        if (part) {
            if (int rc = stage_rows(J.x, O, io())) return rc;
            if (int rc = stage_rows(J.lambda, O, io() + (size_t)N * O)) return rc;
            return stage_statics(io());
        }
        HIPCHK(h, hipMemcpyAsync(io(), J.x, (size_t)N * O * 4, hipMemcpyDefault, st));
        HIPCHK(h, hipMemcpyAsync(io() + (size_t)N * O, J.lambda, (size_t)N * O * 4, hipMemcpyDefault, st));
        HIPCHK(h, to_local(io(), O));
        HIPCHK(h, to_local(io() + (size_t)N * O, O));
        return stage_statics(io());
    }
    int stage_inputs() {
        int rc = MGN_OK;
        switch (J.kind) {
            case JOB_STEP: rc = stage_step(); break;
            case JOB_FORWARD_VJP: rc = stage_forward_vjp(); break;
            case JOB_RHS_VJP: rc = stage_rhs_vjp(); break;
            // the state this step's RHS saw; one-hot node types, val_mask and the normalised edge features were staged once for the sweep
            case JOB_SWEEP_STEP: rc = pad_state(J.x); break;
            // nf_pad, target and (when stale) ef_pad from the resident trajectory: no host array, no gather
            case JOB_DATAPOINT:
                rc = datapoint_stage(h, J.datapoint, J.accumulate, st);
                if (!rc) rc = stage_mask();
                break;
            // the same for B datapoints, from the parent's trajectory into this companion's arena; the mask is listed once
            case JOB_DATAPOINTS:
                rc = datapoints_stage(J.parent, h, J.datapoints, J.B, J.accumulate, st);
                if (!rc) rc = stage_mask_by(J.parent->g.renumbered, T.batch.g2l);
                break;
        }
        if (rc) return rc;
        // further edge sets: the features installed by mgn_set_edge_features, as given (the forward path does not normalise them either)
        for (int q = 1; q < S; ++q)
            if (sx[q].E > 0)
                HIPCHK(h, launch_affine_pad(h->es[q].d_ef.as<float>(), h->es[q].Fe, nullptr, 0, nullptr, nullptr, A + T.ef_pad[q], L, sx[q].E, st));
        return MGN_OK;
    }

    // ---- forward, keeping activations
    // keep = false: first pass of recompute mode -- H1 / H2 / Y are regenerated right before the backward, not stored here
    hipError_t run_fwd(const TrainMlp& m, const TrainFwdArgs& in, int w1sel, const Acts& act, const float* resid, float* out, float* lnout, bool keep) {
        for (int bi = 0; bi < m.nblk; ++bi) {
            const TrainBlock& b = m.b[bi];
            const bool last = bi == m.nblk - 1;
            TrainFwdArgs a;
            const int nin = fwd_unit(m, bi, in, w1sel, Wt, bi > 0 ? A + act.h[bi - 1][2] : nullptr, a);
            if (keep) { a.H1 = A + act.h[bi][0]; a.H2 = A + act.h[bi][1]; a.Y = A + act.h[bi][2]; }
            if (last) { a.resid = resid; a.OUT = out; a.LNOUT = lnout; a.SEG_RCV = in.SEG_RCV; a.SEG_AGG = in.SEG_AGG; a.SEG_CARRY = in.SEG_CARRY; }
            else if (!keep) a.OUT = A + act.h[bi][2];
            a.ln = b.ln ? 1 : 0;
            const bool wide = lnall && last && b.ln;      // whole-array LayerNorm: the kernel stops at Y, statistics and apply follow
            const bool want_stats = wide && (out || lnout) && in.rows > 0;   // (the recomputation of the reverse pass asks for neither: the statistics are kept)
            if (wide) { a.ln = 0; a.resid = nullptr; a.OUT = nullptr; a.LNOUT = nullptr; a.SEG_RCV = nullptr; a.Y = A + act.h[bi][2]; }
            if (want_stats) a.STATS = reinterpret_cast<double*>(A + T.lnpart);   // the kernel leaves (sum, sum of squares) of Y per tile
            if (hipError_t e = launch_mlp_fwd(L, nin, a, st)) return e;
            if (want_stats) {
                float* stats = A + T.lnstats + (size_t)64 * m.lnslot;
                const int64_t n = in.rows * L;
                if (hipError_t e = launch_array_stats_final(a.STATS, train_fwd_stat_slots(L, in.ntiles), n, ln_eps_in, ln_eps_out, stats, st)) return e;
                if (hipError_t e = launch_ln_all_apply(a.Y, stats, Wt + b.tabs + (size_t)T_GAMMA * L, Wt + b.tabs + (size_t)T_BETA * L, resid, out,
                                                       lnout, n, L, st)) return e;
            }
        }
        return hipSuccess;
    }
    hipError_t fwd(const TrainMlp& m, const TrainFwdArgs& in, const Acts& act, const float* resid, float* out, float* lnout, bool keep = true) {
        return run_fwd(m, in, -1, act, resid, out, lnout, keep);
    }
    // edge MLP of step k, set q: [v_s; v_r; e] -> MLP + LayerNorm; with the factored first layer P[s] + Q[r] + e W1e
    // segagg != null: the launch aggregates e' itself (train.h: SEG_*; the caller follows up with launch_seg_fixup)
    hipError_t fwd_edge(int q, int k, const float* resid, float* out, float* lnout, bool keep = true, float* segagg = nullptr) {
        const TrainMlp& m = T.m_pe[q][k];
        const float* v = A + T.Vk[k];
        TrainFwdArgs a = T.factored[q] ? fwd_inputs(sx[q].E, sx[q].nt, A + T.Ek[q][k]) : fwd_inputs(sx[q].E, sx[q].nt, v, sx[q].snd, v, sx[q].rcv, A + T.Ek[q][k]);
        if (segagg) { a.SEG_RCV = sx[q].rcv; a.SEG_AGG = segagg; a.SEG_CARRY = A + T.segcarry; }
        if (!T.factored[q]) return run_fwd(m, a, -1, T.a_pe[q][k], resid, out, lnout, keep);
        Lin2Args p{};                     // (over the halo rows as well: local senders index them)
        p.rows = NT; p.ntiles = nt_t;
        p.X0 = v; p.W0 = Wt + m.b[0].W1[0]; p.W1 = Wt + m.b[0].W1[1];
        p.OUT0 = A + T.Pn; p.OUT1 = A + T.Qn;
        if (hipError_t e = launch_lin2(L, p, st)) return e;
        a.PRE[0] = A + T.Pn; a.preidx[0] = sx[q].snd; a.PRE[1] = A + T.Qn; a.preidx[1] = sx[q].rcv;
        return run_fwd(m, a, 2, T.a_pe[q][k], resid, out, lnout, keep);
    }
    hipError_t fwd_node(int k, const float* resid, float* out, bool keep = true) {
        return fwd(T.m_pn[k], fwd_inputs(N, nt_n, A + T.Vk[k], nullptr, A + T.agg[0][k], nullptr, S > 1 ? A + T.agg[1][k] : nullptr), T.a_pn[k], resid, out,
                   nullptr, keep);
    }

    // The halo exchange of the partitioned step, forward: the owned boundary rows of v go to the peers that list them as halo (packed by
    // the send index; the halo rows are one block behind the owned rows, in the order they arrive).  Reverse: the halo rows of the
    // gradient w.r.t. v go back over the same lists and the owner adds them to its own term (launch_halo_accumulate: a fixed order).
    int halo_forward(float* v) {
        HIPCHK(h, launch_halo_pack(L, v, h->d_send_idx.as<int32_t>(), T.hx_send.as<float>(), (int64_t)g.send_idx.size(), st));
        if (h->comm->a2a_start(T.hx_send.p, T.hx_own_b.data(), T.hx_own_o.data(), T.hx_recv.p, T.hx_halo_b.data(), T.hx_halo_o.data(), st) != 0 ||
            h->comm->a2a_finish(st) != 0)
            return comm_fail("halo exchange");
        HIPCHK(h, launch_halo_unpack(L, T.hx_recv.as<float>(), v + (size_t)N * L, g.n_halo, st));
        return MGN_OK;
    }
    int halo_reverse(float* gv) {
        if (h->comm->a2a_start(gv + (size_t)N * L, T.hx_halo_b.data(), T.hx_halo_o.data(), T.hx_recv.p, T.hx_own_b.data(), T.hx_own_o.data(), st) != 0 ||
            h->comm->a2a_finish(st) != 0)
            return comm_fail("reverse halo exchange");
        HIPCHK(h, launch_halo_accumulate(L, T.hx_recv.as<float>(), acc_row, acc_ptr, acc_pos, gv, T.n_acc, st));
        return MGN_OK;
    }

    // Small meshes replay both launch sequences from hipGraphs (everything they touch lives at fixed addresses in the arena;
    // the inputs, the seed of the reverse pass and the results stay outside).  The captured pointers are checked per call.
    void drop_stale_graphs() {
        if (T.exec_arena == T.arena.p && T.exec_w == T.w.p) return;
        T.drop_graphs();
        T.exec_arena = T.arena.p;
        T.exec_w = T.w.p;
    }
    template <typename F> int graphed(int slot, F&& launches) {
        const bool graphable = h->use_graph && !h->prof && st != nullptr && T.gsets > 1;   // the NULL stream cannot be captured
        return run_graphed(h, st, graphable, T.exec[slot], T.warm[slot], launches);
    }

    int forward() {
        HIPCHK(h, fwd(T.m_en, fwd_inputs(N, nt_n, A + T.nf_pad), T.a_en, nullptr, A + T.Vk[0], nullptr));
        if (part) if (int rc = halo_forward(A + T.Vk[0])) return rc;
        for (int q = 0; q < S; ++q)      // (a partition's ef_pad holds its local edges in the engine's order already)
            HIPCHK(h, fwd(T.m_ee[q], fwd_inputs(sx[q].E, sx[q].nt, A + T.ef_pad[q], part ? nullptr : sx[q].egid), T.a_ee[q], nullptr, A + T.Ek[q][0], nullptr));
        for (int k = 0; k < mps; ++k) {
            for (int q = 0; q < S; ++q) {
                if (!lnall && sx[q].E > 0 && train_fwd_fused_agg(L, sx[q].nt)) {   // aggregation inside the edge launch (large meshes)
                    HIPCHK(h, fwd_edge(q, k, A + T.Ek[q][k], A + T.Ek[q][k + 1], nullptr, T.kept(k, mps), A + T.agg[q][k]));
                    HIPCHK(h, launch_seg_fixup(L, sx[q].rowptr, A + T.segcarry, A + T.agg[q][k], (int32_t)N, st));
                    continue;
                }
                HIPCHK(h, fwd_edge(q, k, A + T.Ek[q][k], A + T.Ek[q][k + 1], A + T.Enew, T.kept(k, mps)));
                HIPCHK(h, launch_segment_sum(L, A + T.Enew, sx[q].rowptr, nullptr, nullptr, A + T.agg[q][k], (int32_t)N, st));
            }
            HIPCHK(h, fwd_node(k, A + T.Vk[k], A + T.Vk[k + 1], T.kept(k, mps)));
            if (part && k + 1 < mps) if (int rc = halo_forward(A + T.Vk[k + 1])) return rc;   // (the decoder reads owned rows only)
        }
        HIPCHK(h, fwd(T.m_de, fwd_inputs(N, nt_n, A + T.Vk[mps]), T.a_de, nullptr, nullptr, nullptr));
        return MGN_OK;
    }

    // ---- seed of the reverse pass
    int seed() {
        const size_t y_out = T.a_de.h[T.m_de.nblk - 1][2];        // the decoder's output (its last unit's Y)
        nlb = vjp() ? 0 : loss_blocks(T.mask_n);
        HIPCHK(h, hipMemsetAsync(A + T.Gout, 0, (size_t)N * L * 4, st));
        if (J.kind == JOB_DATAPOINTS) {   // the mean over the B copies of the masked loss of each, and its gradient: per-copy partials, one fold
            HIPCHK(h, T.loss.ensure((size_t)J.B * nlb * sizeof(double)));
            HIPCHK(h, T.batch.out.ensure((size_t)(J.B + 1) * 4));
            HIPCHK(h, launch_loss_batch(A + y_out, L, T.target.as<float>(), O, T.mask.as<int32_t>(), T.mask_n, N / J.B, J.B,
                                        J.parent->g.renumbered ? 0 : J.mask_index_base, A + T.Gout, T.loss.as<double>(), T.batch.out.as<float>(), st));
        } else if (!vjp()) {   // loss = mean(mse_reduce(target, out)[mask]) and its gradient w.r.t. out
            HIPCHK(h, T.loss.ensure((size_t)nlb * sizeof(double)));
            HIPCHK(h, launch_loss(A + y_out, L, T.target.as<float>(), O, T.mask.as<int32_t>(), T.mask_n, J.nmask, renum ? 0 : J.mask_index_base,
                                  A + T.Gout, T.loss.as<double>(), st));
        } else if (J.kind == JOB_FORWARD_VJP) {   // the cotangent of the model's output as given
            HIPCHK(h, launch_vjp_seed(A + y_out, L, O, io() + (size_t)N * O, nullptr, nullptr, nullptr, A + T.Gout,
                                      J.out ? T.target.as<float>() : nullptr, N, st));
        } else {        // dx/dt = inverse_data(o_norm, out) .* val_mask  =>  d/d out = lambda .* val_mask .* out_scale
            const float* os = h->have_onorm ? nrm + 2 * c.Fn + 2 * c.Fe : nullptr;
            const float* vm = J.val_mask ? io() + (size_t)N * (O + c.Fn) : nullptr;
            HIPCHK(h, launch_vjp_seed(A + y_out, L, O, io() + (size_t)N * O, vm, os, os ? os + O : nullptr, A + T.Gout,
                                      J.dxdt ? T.target.as<float>() : nullptr, N, st));
        }
        return MGN_OK;
    }

    // ---- backward
    int second_stream() {   // (created outside of any capture)
        if (!overlap || T.aux) return MGN_OK;
        HIPCHK(h, hipStreamCreateWithFlags(&T.aux, hipStreamNonBlocking));
        HIPCHK(h, hipEventCreateWithFlags(&T.ev_bwd, hipEventDisableTiming));
        for (hipEvent_t& e : T.ev_wg) HIPCHK(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        return MGN_OK;
    }
    // The parameter gradients of a launch unit are one k_wgrad launch and one k_reduce_partials launch behind its activation backward.
    // Small meshes (overlap): the pair of unit i only reads what k_mlp_bwd left in gradient-buffer set i % gsets and the kept activations,
    // and runs on a second stream beside the activation backward of the next units.  Not in recompute mode (there the kept activations
    // are shared buffers which the next step's recomputation overwrites) and not on large meshes, which fill the chip on their own
    // (prepare_graph).  The reverse pass is issued twice per handle -- eagerly, then under stream capture -- and both must issue the same
    // launches: n_bwd is all the state that passes from unit to unit, and backward() sets it.
    // The buffer set of the next activation backward, free to be written: its last occupant's weight gradients have run.  ev_wg[gs] is
    // recorded once per unit in set gs.  The second stream is in order and a set comes round again only gsets units later, so the record
    // of unit i - gsets is the last one issued when unit i waits here, and the next one (unit i's own) is issued behind this wait: no
    // wait can see a re-recorded event.
    int wgrad_acquire(int& gs) {
        gs = overlap ? n_bwd % T.gsets : 0;
        if (overlap && n_bwd >= T.gsets) HIPCHK(h, hipStreamWaitEvent(st, T.ev_wg[gs], 0));
        ++n_bwd;
        return MGN_OK;
    }
    int wgrad_unit(const WgradUnit& u) {
        const TrainBlock& b = u.b;
        const int gs = u.gs;
        const int64_t rows = u.rows;
        const int64_t lrows_u = rows > u.node_rows ? rows : u.node_rows;   // a launch covers its longest job (node jobs of a factored edge MLP)
        const int64_t lrows = overlap ? lrows_all : lrows_u;               // (second stream: the longest job of the model; 128-row blocks either way)
        const int nb = wgrad_blocks(lrows);
        T.wg_rpb_last = wgrad_rows_per_block(lrows);
        const hipStream_t wst = overlap ? T.aux : st;
        if (overlap) {
            HIPCHK(h, hipEventRecord(T.ev_bwd, st));
            HIPCHK(h, hipStreamWaitEvent(wst, T.ev_bwd, 0));
        }
        if (nb > 0 && lrows_u > 0) {
            WgradBatch wb{};
            ReduceBatch rb{};
            int nw = 0;                                    // partial-dW regions taken
            auto job = [&](const float* X, const int32_t* xi_, const float* Gm, long woff, int nrows, int cols, long boff, int bcols, int64_t jrows = -1) {
                if (woff < 0 && boff < 0) return;          // identity slot
                WgradJob& j = wb.job[wb.njobs];
                if (jrows < 0) jrows = rows;
                const int nbj = wgrad_blocks_of_job(lrows, jrows);     // blocks of this launch that hold rows of the job
                j.X = X; j.xidx = xi_; j.G = Gm; j.rows = jrows;
                j.pw = woff >= 0 ? A + T.pw + (size_t)nw * nb * L * L : nullptr;
                j.pb = boff >= 0 ? A + T.pb + (size_t)wb.njobs * nb * L : nullptr;
                if (woff >= 0) {
                    rb.job[rb.njobs++] = ReduceJob{j.pw, nbj, (int64_t)L * L, nrows, cols, L, G + woff};
                    ++nw;
                }
                if (boff >= 0) rb.job[rb.njobs++] = ReduceJob{j.pb, nbj, (int64_t)L, 1, bcols, L, G + boff};
                ++wb.njobs;
            };
            job(A + u.hb[1], nullptr, A + T.GY[gs], b.gW[2], L, b.out_cols, b.gb[2], b.out_cols);
            job(A + u.hb[0], nullptr, A + T.GZ2[gs], b.gW[1], L, L, b.gb[1], L);
            if (u.io.fq < 0) {
                for (int j = 0; j < b.nin; ++j)
                    job(u.io.xin[j], u.io.xi[j], A + T.GZ1[gs], b.gW[0] + (long)j * L * L, b.in_rows, L, j == 0 ? b.gb[0] : -1, L);
            } else {   // dW1e = e^T GZ1 (+ db1) over the edges; dW1s = v^T SGs, dW1r = v^T SGr over the nodes
                job(u.io.xin[0], u.io.xi[0], A + T.GZ1[gs], b.gW[0] + (long)2 * L * L, L, L, b.gb[0], L);
                job(u.io.vin, nullptr, A + T.SGs, b.gW[0], L, L, -1, L, u.node_rows);
                job(u.io.vin, nullptr, A + T.SGr, b.gW[0] + (long)L * L, L, L, -1, L, N);
            }
            if (u.lnsum) {
                const int ng = std::min(LNSUM_GROUPS, (int)((u.ntiles + 7) / 8));
                rb.job[rb.njobs++] = ReduceJob{A + T.lnsum2, ng, (int64_t)2 * L, 1, L, L, G + b.gbeta};
                rb.job[rb.njobs++] = ReduceJob{A + T.lnsum2 + L, ng, (int64_t)2 * L, 1, L, L, G + b.ggamma};
            } else if (b.ln && !u.wide) {
                job(nullptr, nullptr, A + T.GXH[gs], -1, 0, 0, b.ggamma, L);
                job(nullptr, nullptr, A + T.GT[gs], -1, 0, 0, b.gbeta, L);
            }
            HIPCHK(h, launch_wgrad(L, wb, lrows, wst));
            HIPCHK(h, launch_reduce_partials(rb, wst));
        }
        if (overlap) HIPCHK(h, hipEventRecord(T.ev_wg[gs], wst));
        return MGN_OK;
    }
    int wgrad_join() {   // the second stream is in order: the event of its last unit covers all of it
        if (overlap && n_bwd > 0) HIPCHK(h, hipStreamWaitEvent(st, T.ev_wg[(n_bwd - 1) % T.gsets], 0));
        return MGN_OK;
    }
    // activation backward of one launch unit (kept activations hb) + all of its parameter gradients
    int bwd_unit(const TrainBlock& b, int64_t rows, int32_t ntiles, const size_t (&hb)[3], const BwdIo& io_, int lnslot) {
        const int fq = io_.fq;
        const bool fact = fq >= 0;
        const bool wide = lnall && b.ln;
        const int64_t node_rows = fact ? NT : 0;          // rows that send: SGs, dW1s (halo rows included); SGr and dW1r stop at the N owned rows
        const int nin_k = fact ? 1 : b.nin;               // input blocks the kernel unwinds
        int gs = 0;
        if (int rc = wgrad_acquire(gs)) return rc;
        TrainBwdArgs a{};
        a.rows = rows; a.ntiles = ntiles;
        a.G0 = io_.g0; a.G1 = io_.g1; a.g1idx = io_.g1i;
        a.H1 = A + hb[0]; a.H2 = A + hb[1]; a.Y = A + hb[2];
        a.W3T = Wt + b.W3T; a.W2T = Wt + b.W2T;
        for (int j = 0; j < nin_k; ++j) {
            const int jw = fact ? 2 : j;                   // factored: block 2 (e) of W1
            a.W1T[j] = (b.has_w1t && io_.gx[j]) ? Wt + b.W1T[jw] : nullptr;
            a.GX[j] = io_.gx[j];
            a.GXadd[j] = io_.gxadd[j];
        }
        a.tabs = Wt + b.tabs;
        a.ln = b.ln ? 1 : 0;
        a.GT = A + T.GT[gs]; a.GXH = A + T.GXH[gs]; a.GY = A + T.GY[gs]; a.GZ2 = A + T.GZ2[gs]; a.GZ1 = A + T.GZ1[gs];
        // LayerNorm-parameter sums: inside the eight-tile backward kernel (per block), else GT / G xhat rows written here feed two column-sum jobs
        const bool lnsum = b.ln && !wide && !overlap && rows > 0 && train_bwd_ln_sums(L, ntiles);
        if (lnsum) { a.GT = nullptr; a.GXH = nullptr; a.LNSUM = A + T.lnsum; }
        if (b.ln && !wide && !lnsum && !T.need_gt && rows > 0) return fail(h, MGN_E_STATE, "training arena laid out without GT / GXH rows but a launch unit needs them");
        if (wide && rows > 0) {   // pullback of the whole-array LayerNorm: dgamma, dbeta and the two means first (two column reductions)
            HIPCHK(h, launch_lnall_bwd(io_.g0, io_.g1, io_.g1i, A + hb[2], A + T.lnstats + (size_t)64 * lnslot, Wt + b.tabs + (size_t)T_GAMMA * L, rows, L,
                                       reinterpret_cast<double*>(A + T.lnpart), A + T.lnm, G + b.ggamma, G + b.gbeta, st));
            a.ln = 2;                   // the kernel maps G to the gradient at Y as it loads it
            a.LNS = A + T.lnstats + (size_t)64 * lnslot;
            a.LNM = A + T.lnm;
        }
        HIPCHK(h, launch_mlp_bwd(L, nin_k, a, st));
        if (lnsum)    // [blocks][2 L] -> [LNSUM_GROUPS][2 L], in order; the unit's reduction launch adds the groups
            HIPCHK(h, launch_colsum_groups(A + T.lnsum, (ntiles + 7) / 8, 2 * L, LNSUM_GROUPS, A + T.lnsum2, st));
        if (fact) {   // gather <-> segmented-sum duality on GZ1 itself: SGr[n] = sum of GZ1 over edges received by n, SGs: sent by n
            HIPCHK(h, launch_segment_sum_pair(L, A + T.GZ1[gs], sx[fq].rowptr, sx[fq].rowptr_s, sx[fq].perm_s, A + T.SGr, A + T.SGs, (int32_t)N, st));
            HIPCHK(h, launch_segment_sum(L, A + T.GZ1[gs], sx[fq].rowptr_s + N, sx[fq].perm_s, nullptr, A + T.SGs + (size_t)N * L, g.n_halo, st));
            if (g.n_halo > 0) HIPCHK(h, hipMemsetAsync(A + T.SGr + (size_t)N * L, 0, (size_t)g.n_halo * L * 4, st));   // (a halo row receives nothing here)
        }
        return wgrad_unit(WgradUnit{b, io_, hb, rows, node_rows, ntiles, gs, wide, lnsum});
    }
    // one MLP: its second unit (if any) first, handing the gradient w.r.t. its input to the first through GXB
    int bwd(const TrainMlp& m, int64_t rows, int32_t ntiles, const Acts& act, const BwdIo& io_) {
        if (m.nblk == 1) return bwd_unit(m.b[0], rows, ntiles, act.h[0], io_, m.lnslot);
        BwdIo u1, u0 = io_;
        u1.g0 = io_.g0; u1.g1 = io_.g1; u1.g1i = io_.g1i;
        u1.gx[0] = A + T.GXB; u1.xin[0] = A + act.h[0][2];
        if (int rc = bwd_unit(m.b[1], rows, ntiles, act.h[1], u1, m.lnslot)) return rc;
        u0.g0 = A + T.GXB; u0.g1 = nullptr; u0.g1i = nullptr;
        return bwd_unit(m.b[0], rows, ntiles, act.h[0], u0, m.lnslot);
    }
    // the edge MLP of step k, set q: d loss / d e_{k+1} in gE[ecur], d loss / d agg_k in gAgg -> gE[ecur ^ 1], and its share of gV[nxt]
    int bwd_edge(int q, int k, int nxt, int ecur) {
        const TrainMlp& me = T.m_pe[q][k];
        const int64_t E = sx[q].E;
        const int enxt = ecur ^ 1;
        BwdIo u;
        u.g0 = A + T.gE[q][ecur]; u.g1 = A + T.gAgg[q]; u.g1i = sx[q].rcv;
        if (!T.factored[q]) {   // edge MLP: e' feeds e_{k+1} = e_k + e' and agg_k[receiver]
            u.gx[0] = A + T.GXs; u.gx[1] = A + T.GXr; u.gx[2] = A + T.gE[q][enxt];
            u.gxadd[2] = A + T.gE[q][ecur];
            u.xin[0] = A + T.Vk[k]; u.xin[1] = A + T.Vk[k]; u.xin[2] = A + T.Ek[q][k];
            u.xi[0] = sx[q].snd; u.xi[1] = sx[q].rcv;
            if (int rc = bwd(me, E, sx[q].nt, T.a_pe[q][k], u)) return rc;
            T.wg_rpb_edge[q] = T.wg_rpb_last;
            // gather duality: the gradients of v[receivers] / v[senders] are segmented sums over the receiver / sender CSR
            HIPCHK(h, launch_segment_sum2(L, A + T.GXr, sx[q].rowptr, A + T.GXs, sx[q].rowptr_s, sx[q].perm_s, A + T.gV[nxt], A + T.gV[nxt],
                                          (int32_t)N, st));
            // halo rows only send
            HIPCHK(h, launch_segment_sum(L, A + T.GXs, sx[q].rowptr_s + N, sx[q].perm_s, nullptr, A + T.gV[nxt] + (size_t)N * L, g.n_halo, st));
        } else {             // factored first layer: per edge only the e block; the v blocks per node from SGs / SGr
            u.gx[0] = A + T.gE[q][enxt];
            u.gxadd[0] = A + T.gE[q][ecur];
            u.xin[0] = A + T.Ek[q][k];
            u.fq = q; u.vin = A + T.Vk[k];
            if (int rc = bwd(me, E, sx[q].nt, T.a_pe[q][k], u)) return rc;
            T.wg_rpb_edge[q] = T.wg_rpb_last;
            if (g.n_halo > 0) HIPCHK(h, hipMemsetAsync(A + T.gV[nxt] + (size_t)N * L, 0, (size_t)g.n_halo * L * 4, st));   // (no node MLP wrote them)
            Lin2Args l2{};    // gV += SGs W1s^T + SGr W1r^T
            l2.rows = NT; l2.ntiles = nt_t;
            l2.X0 = A + T.SGs; l2.X1 = A + T.SGr; l2.W0 = Wt + me.b[0].W1T[0]; l2.W1 = Wt + me.b[0].W1T[1];
            l2.ADD = A + T.gV[nxt]; l2.OUT0 = A + T.gV[nxt];
            HIPCHK(h, launch_lin2(L, l2, st));
        }
        if (E == 0) HIPCHK(h, hipMemsetAsync(A + T.gE[q][enxt], 0, (size_t)L * 4, st));
        return MGN_OK;
    }
    int backward() {
        n_bwd = 0;
        HIPCHK(h, hipMemsetAsync(G, 0, h->params.size() * 4, st));   // (inside the replayed sequence: G is the engine's own buffer)
        int cur = 0, ecur = 0;   // gV[cur], gE[q][ecur] hold the gradients w.r.t. the latents entering the part of the model already unwound
        {
            BwdIo u;
            u.g0 = A + T.Gout; u.gx[0] = A + T.gV[cur]; u.xin[0] = A + T.Vk[mps];
            if (int rc = bwd(T.m_de, N, nt_n, T.a_de, u)) return rc;
        }
        for (int q = 0; q < S; ++q) HIPCHK(h, hipMemsetAsync(A + T.gE[q][ecur], 0, (size_t)(sx[q].E > 0 ? sx[q].E : 1) * L * 4, st));
        for (int k = mps - 1; k >= 0; --k) {
            const int nxt = cur ^ 1;
            if (!T.kept(k, mps)) {   // regenerate H1, H2, Y of the MLPs of this step from their kept inputs
                HIPCHK(h, fwd_node(k, nullptr, nullptr));
                for (int q = 0; q < S; ++q) HIPCHK(h, fwd_edge(q, k, nullptr, nullptr, nullptr));
            }
            {   // node MLP: v_{k+1} = v_k + MLP_v([v_k; agg_k (per set)])
                BwdIo u;
                u.g0 = A + T.gV[cur];
                u.gx[0] = A + T.gV[nxt]; u.gx[1] = A + T.gAgg[0]; u.gx[2] = S > 1 ? A + T.gAgg[1] : nullptr;
                u.gxadd[0] = A + T.gV[cur];
                u.xin[0] = A + T.Vk[k]; u.xin[1] = A + T.agg[0][k]; u.xin[2] = S > 1 ? A + T.agg[1][k] : nullptr;
                if (int rc = bwd(T.m_pn[k], N, nt_n, T.a_pn[k], u)) return rc;
                T.wg_rpb_node = T.wg_rpb_last;
            }
            for (int q = 0; q < S; ++q)
                if (int rc = bwd_edge(q, k, nxt, ecur)) return rc;
            // the halo rows' share of d loss / d v_k joins the owners' before node MLP k - 1 (the node encoder for k = 0) is unwound
            if (part) if (int rc = halo_reverse(A + T.gV[nxt])) return rc;
            cur = nxt;
            ecur ^= 1;
        }
        {
            BwdIo u;
            u.g0 = A + T.gV[cur]; u.gx[0] = vjp() ? A + T.gNF : nullptr; u.xin[0] = A + T.nf_pad;
            if (int rc = bwd(T.m_en, N, nt_n, T.a_en, u)) return rc;
        }
        for (int q = 0; q < S; ++q) {
            BwdIo u;
            u.g0 = A + T.gE[q][ecur]; u.xin[0] = A + T.ef_pad[q]; u.xi[0] = part ? nullptr : sx[q].egid;
            if (int rc = bwd(T.m_ee[q], sx[q].E, sx[q].nt, T.a_ee[q], u)) return rc;
        }
        return wgrad_join();
    }

    // ---- results
    // Finish of a partition: every rank's gradient and loss numerator are gathered and added in ascending rank order, in double, by the same
    // kernel on every rank: the same bits everywhere.  The call's one blocking point follows.
    int finish_partition() {
        const int64_t np = (int64_t)h->params.size();
        double num = 0.0;
        HIPCHK(h, launch_loss_numerator(T.loss.as<double>(), nlb, T.fin_s.as<double>(), st));
        if (h->comm->allgather(T.fin_s.p, (size_t)rank_sum_stride(np) * 4, T.fin_r.p, st) != 0) return comm_fail("allgather of the gradients");
        HIPCHK(h, launch_rank_sum(T.fin_r.as<float>(), c.nranks, np, T.grads.as<float>(), T.fin_loss.as<double>(), st));
        HIPCHK(h, hipMemcpyAsync(J.grads, T.grads.p, (size_t)np * 4, hipMemcpyDefault, st));
        HIPCHK(h, hipMemcpyAsync(&num, T.fin_loss.p, sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(h, hipStreamSynchronize(st));
        *J.loss = (float)(num / (double)J.nmask);
        return MGN_OK;
    }
    // Finish of a VJP on a partition: the ranks' gradients through finish_partition's float exchange without its loss part (the head of
    // this rank's part is zeroed: mgn_step leaves its loss numerator there), then the per-node results row by row through
    // gather_rows_global, which blocks: complete arrays in the caller's order on every rank.
    int finish_partition_vjp() {
        const int64_t np = (int64_t)h->params.size();
        HIPCHK(h, hipMemsetAsync(T.fin_s.p, 0, (size_t)RANK_SUM_HEAD * 4, st));
        if (h->comm->allgather(T.fin_s.p, (size_t)rank_sum_stride(np) * 4, T.fin_r.p, st) != 0) return comm_fail("allgather of the gradients");
        HIPCHK(h, launch_rank_sum(T.fin_r.as<float>(), c.nranks, np, T.grads.as<float>(), T.fin_loss.as<double>(), st));
        HIPCHK(h, hipMemcpyAsync(J.grads, T.grads.p, (size_t)np * 4, hipMemcpyDefault, st));
        if (J.kind == JOB_FORWARD_VJP) {
            HIPCHK(h, launch_extract_cols(A + T.gNF, L, c.Fn, nullptr, io(), N, st));
            if (int rc = gather_rows_global(h, io(), c.Fn, J.nfbar)) return rc;
            if (J.out) if (int rc = gather_rows_global(h, T.target.as<float>(), O, J.out)) return rc;
        } else {
            HIPCHK(h, launch_extract_cols(A + T.gNF, L, O, h->have_nnorm ? nrm : nullptr, io(), N, st));
            if (int rc = gather_rows_global(h, io(), O, J.xbar)) return rc;
            if (J.dxdt) if (int rc = gather_rows_global(h, T.target.as<float>(), O, J.dxdt)) return rc;
        }
        return MGN_OK;
    }
    // a per-node result [N][width] of a VJP: back into the caller's order and out
    int give(float* buf, int width, float* user) {
        HIPCHK(h, to_global(buf, width));
        HIPCHK(h, hipMemcpyAsync(user, buf, (size_t)N * width * 4, hipMemcpyDefault, st));
        return MGN_OK;
    }
    int results() {
        if (J.kind == JOB_SWEEP_STEP) {     // xbar (engine order) into io for the adjoint kernel; the step's gradient into the double accumulator
            HIPCHK(h, launch_extract_cols(A + T.gNF, L, O, h->have_nnorm ? nrm : nullptr, io(), N, st));
            HIPCHK(h, launch_grad_accum(G, J.gacc, (int64_t)h->params.size(), J.first, st));
            return MGN_OK;
        }
        if (part) return vjp() ? finish_partition_vjp() : finish_partition();
        if (J.kind == JOB_DATAPOINTS) {     // the fold kernel rounded every loss once: [loss_0 .. loss_{B-1} | mean]
            std::vector<float> lo((size_t)J.B + 1);
            HIPCHK(h, hipMemcpyAsync(J.grads, G, h->params.size() * 4, hipMemcpyDefault, st));
            HIPCHK(h, hipMemcpyAsync(lo.data(), T.batch.out.p, lo.size() * 4, hipMemcpyDeviceToHost, st));
            HIPCHK(h, hipStreamSynchronize(st));
            *J.loss = lo[(size_t)J.B];
            if (J.losses) memcpy(J.losses, lo.data(), (size_t)J.B * 4);
            return MGN_OK;
        }
        std::vector<double> lp((size_t)nlb);
        HIPCHK(h, hipMemcpyAsync(J.grads, G, h->params.size() * 4, hipMemcpyDefault, st));
        if (!vjp()) {
            HIPCHK(h, hipMemcpyAsync(lp.data(), T.loss.p, lp.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        } else if (J.kind == JOB_FORWARD_VJP) {
            HIPCHK(h, launch_extract_cols(A + T.gNF, L, c.Fn, nullptr, io(), N, st));
            if (int rc = give(io(), c.Fn, J.nfbar)) return rc;
            if (J.out) if (int rc = give(T.target.as<float>(), O, J.out)) return rc;
        } else {
            // x enters through the node normaliser: xbar = (d / d nf)[:, 0:O] .* node_scale[0:O]
            HIPCHK(h, launch_extract_cols(A + T.gNF, L, O, h->have_nnorm ? nrm : nullptr, io(), N, st));
            if (int rc = give(io(), O, J.xbar)) return rc;
            if (J.dxdt) if (int rc = give(T.target.as<float>(), O, J.dxdt)) return rc;
        }
        HIPCHK(h, hipStreamSynchronize(st));
        if (!vjp()) {
            double s = 0.0;
            for (double v : lp) s += v;
            *J.loss = (float)(s / (double)J.nmask);
        }
        return MGN_OK;
    }
};

int train_run(mgn_handle* h, const TrainJob& J) {
    TrainPass P(h, J);
    if (int rc = P.stage_inputs()) return rc;
    P.drop_stale_graphs();
    if (int rc = P.graphed(0, [&] { return P.forward(); })) return rc;
    if (int rc = P.seed()) return rc;
    if (int rc = P.second_stream()) return rc;
    if (int rc = P.graphed(P.vjp() ? 2 : 1, [&] { return P.backward(); })) return rc;
    return P.results();
}

}  // namespace

// The hooks of mgn_group_step_datapoints (engine_internal.h).  The checks are those of mgn_step_datapoint (share == 1) and of
// mgn_step_datapoints at B > 1 (share > 1) below, in their order and with their statuses, less everything that launches or allocates.
namespace mgn {
int step_datapoints_check(mgn_engine* h, const char* who, const int32_t* datapoints, int32_t B, int32_t share, const int32_t* mask, int64_t nmask,
                          int32_t mask_index_base, size_t n_grads) {
    if (int rc = datapoint_need(h, who, true, true)) return rc;
    const mgn_config& c = h->cfg;
    if (share > 1 && c.nranks != 1) return fail(h, MGN_E_STATE, "%s with B > 1 drives one partition", who);
    const int32_t T_ = h->train->traj.T;
    for (int32_t b = 0; b < B; ++b)
        if (datapoints[b] < 0 || datapoints[b] > T_ - 2)
            return fail(h, MGN_E_ARG, "%s: datapoint %d (entry %d) outside [0, %d]", who, (int)datapoints[b], (int)b, (int)T_ - 2);
    if (nmask < 1) return fail(h, MGN_E_ARG, "%s: empty mask", who);
    if (mask_index_base != 0 && mask_index_base != 1) return fail(h, MGN_E_ARG, "%s: mask_index_base must be 0 or 1", who);
    const int64_t n_nodes = c.nranks > 1 ? h->g.N : h->g.n_own;          // (a partition takes the mask of the whole mesh)
    for (int64_t i = 0; i < nmask; ++i) {
        const int64_t n = (int64_t)mask[i] - mask_index_base;
        if (n < 0 || n >= n_nodes) return fail(h, MGN_E_ARG, "%s: mask entry %lld out of range", who, (long long)i);
    }
    if (share > 1) {
        const int64_t N = h->g.n_own, E = h->g.set[0].e_local;
        if ((int64_t)share * N > INT32_MAX || (int64_t)share * E > INT32_MAX)
            return fail(h, MGN_E_ARG, "%s: %d copies of %lld nodes and %lld edges overflow int32 ids", who, (int)share, (long long)N, (long long)E);
        if (h->nsets != 1) return fail(h, MGN_E_UNSUPPORTED, "%s with a share of more than one datapoint takes one edge set (the companion replicates one)", who);
        if (c.ln_dims == MGN_LN_ALL)
            return fail(h, MGN_E_UNSUPPORTED, "%s with a share of more than one datapoint and ln_dims = MGN_LN_ALL: whole-array statistics would span the batch, a different model", who);
    }
    if (int rc = need(h, true, true, false, true)) return rc;
    if (c.nranks != 1 && h->nsets != 1) return fail(h, MGN_E_UNSUPPORTED, "%s on a partitioned mesh takes one edge set", who);
    for (int q = 1; q < h->nsets; ++q)
        if (h->g.set[q].E > 0 && !h->es[q].have_ef)
            return fail(h, MGN_E_STATE, "edge set %d has edges but no features: call mgn_set_edge_features after mgn_set_edge_set", q);
    if (n_grads != h->params.size()) return fail(h, MGN_E_ARG, "%s: grads has %zu floats, model has %zu", who, n_grads, h->params.size());
    return MGN_OK;
}
int datapoint_accumulate(mgn_engine* h, int32_t t) { return datapoint_norms(h, t, true, h->stream); }
}  // namespace mgn

extern "C" int mgn_step(mgn_handle* h, const float* nf, const float* ef, const float* target, const int32_t* mask, int64_t nmask,
                        int32_t mask_index_base, float* grads, size_t n_grads, float* loss) try {
    if (!h) return MGN_E_ARG;
    if (!nf || !target || !mask || !grads || !loss) return fail(h, MGN_E_ARG, "mgn_step: null argument");
    if (int rc = train_prepare(h, "mgn_step", n_grads, true)) return rc;
    if (!ef && h->g.set[0].E > 0) return fail(h, MGN_E_ARG, "mgn_step: null argument");
    if (nmask < 1) return fail(h, MGN_E_ARG, "mgn_step: empty mask");
    if (mask_index_base != 0 && mask_index_base != 1) return fail(h, MGN_E_ARG, "mgn_step: mask_index_base must be 0 or 1");
    const int64_t n_nodes = h->cfg.nranks > 1 ? h->g.N : h->g.n_own;      // (a partition takes the mask of the whole mesh)
    for (int64_t i = 0; i < nmask; ++i) {
        const int64_t n = (int64_t)mask[i] - mask_index_base;
        if (n < 0 || n >= n_nodes) return fail(h, MGN_E_ARG, "mgn_step: mask entry %lld out of range", (long long)i);
    }
    TrainJob J;
    J.nf = nf; J.ef = ef; J.target = target; J.mask = mask; J.nmask = nmask; J.mask_index_base = mask_index_base;
    J.loss = loss; J.grads = grads;
    return train_run(h, J);
} MGN_CATCH(h)

// ---- Derivative training on a resident trajectory (reference src/MeshGraphNets.jl:364-378 over src/strategies.jl:395-416) ----
extern "C" int mgn_train_set_trajectory(mgn_handle* h, const float* frames, int32_t T_, const float* times, float dt,
                                        const float* node_type_onehot, const float* ef_raw) try {
    const char* who = "mgn_train_set_trajectory";
    if (!h) return MGN_E_ARG;
    if (int rc = datapoint_need(h, who, true, false)) return rc;
    const mgn_config& c = h->cfg;
    const bool part = c.nranks > 1;    // every rank is given the arrays of the whole mesh and keeps the rows it owns
    const int64_t N = h->g.n_own, E = h->g.set[0].e_local, NG = part ? h->g.N : N, EG = part ? h->g.set[0].E : E;
    if (!frames) return fail(h, MGN_E_ARG, "%s: null argument", who);
    if (T_ < 2) return fail(h, MGN_E_ARG, "%s: a trajectory has at least two frames, got %d", who, (int)T_);
    if (c.Fn < c.O) return fail(h, MGN_E_ARG, "%s: Fn < O", who);
    if ((c.Fn > c.O && !node_type_onehot) || (!ef_raw && EG > 0)) return fail(h, MGN_E_ARG, "%s: null argument", who);
    std::vector<float> delta((size_t)T_ - 1, dt);
    if (times) {
        std::vector<float> tm((size_t)T_);
        HIPCHK(h, hipMemcpy(tm.data(), times, (size_t)T_ * 4, hipMemcpyDefault));
        for (int32_t t = 0; t + 1 < T_; ++t) delta[(size_t)t] = tm[(size_t)t + 1] - tm[(size_t)t];
    }
    for (int32_t t = 0; t + 1 < T_; ++t)
        if (!(delta[(size_t)t] != 0.f)) return fail(h, MGN_E_ARG, "%s: the time step of datapoint %d is zero (or not a number)", who, (int)t);
    TrainState::Trajectory& R = h->train->traj;
    R.have = false; R.ef_pad_ok = false; R.ef_sums_ok = false;
    ++R.ef_gen;
    const hipStream_t st = h->stream;
    const size_t fl = (size_t)T_ * (size_t)N * c.O, ol = (size_t)N * (c.Fn - c.O), el = (size_t)E * c.Fe;
    HIPCHK(h, R.frames.ensure(fl * 4));
    HIPCHK(h, R.onehot.ensure(ol * 4));
    HIPCHK(h, R.ef_raw.ensure(el * 4));
    if (part) {
        // The mesh's arrays pass through a staging buffer whose size does not grow with T: a whole number of frames of the mesh (at least
        // one; MGN_TRAJ_STAGE_BYTES, 64 MB) per pass, or the one-hot rows, or the edge features.  Each pass is gathered into the rows this rank
        // owns -- frames and one-hot rows by own_gid, the local edges by edge_gid, in the engine's order: datapoint_stage's launch_affine_pad
        // then leaves in ef_pad what stage_features gathers out of a caller's [E][Fe] array.
        const int32_t* gid = h->d_own_gid.as<int32_t>();
        const size_t frame = (size_t)NG * c.O, olg = (size_t)NG * (c.Fn - c.O), elg = (size_t)EG * c.Fe;
        const size_t budget = (size_t)std::max(4, env_int("MGN_TRAJ_STAGE_BYTES", 64 << 20)) / 4;   // floats
        const int64_t per = std::max<int64_t>(1, std::min<int64_t>(T_, frame ? (int64_t)(budget / frame) : T_));
        std::vector<int32_t> egid((size_t)E);
        for (int64_t i = 0; i < E; ++i) egid[(size_t)i] = (int32_t)h->g.set[0].edge_gid[(size_t)i];
        HIPCHK(h, h->stage.ensure((std::max({(size_t)per * frame, olg, elg}) + (size_t)E) * 4));
        float* stg = h->stage.as<float>();
        int32_t* d_egid = reinterpret_cast<int32_t*>(stg + std::max({(size_t)per * frame, olg, elg}));
        for (int64_t f0 = 0; f0 < T_; f0 += per) {
            const int64_t nf = std::min<int64_t>(per, T_ - f0);
            HIPCHK(h, hipMemcpyAsync(stg, frames + (size_t)f0 * frame, (size_t)nf * frame * 4, hipMemcpyDefault, st));
            for (int64_t j = 0; j < nf; ++j)
                HIPCHK(h, launch_permute_rows(R.frames.as<float>() + (size_t)(f0 + j) * (size_t)N * c.O, stg + (size_t)j * frame, gid, N, c.O, false, st));
        }
        if (ol) {
            HIPCHK(h, hipMemcpyAsync(stg, node_type_onehot, olg * 4, hipMemcpyDefault, st));
            HIPCHK(h, launch_permute_rows(R.onehot.as<float>(), stg, gid, N, c.Fn - c.O, false, st));
        }
        if (el) {
            HIPCHK(h, hipMemcpyAsync(d_egid, egid.data(), (size_t)E * 4, hipMemcpyHostToDevice, st));
            HIPCHK(h, hipMemcpyAsync(stg, ef_raw, elg * 4, hipMemcpyDefault, st));
            HIPCHK(h, launch_affine_pad_gather(stg, c.Fe, nullptr, 0, nullptr, nullptr, d_egid, R.ef_raw.as<float>(), c.Fe, E, st));
        }
    } else if (h->g.renumbered) {      // into the engine's node order once, here: no gather per step
        const int32_t* gid = h->d_own_gid.as<int32_t>();
        HIPCHK(h, h->stage.ensure(std::max(fl, ol) * 4));
        HIPCHK(h, hipMemcpyAsync(h->stage.p, frames, fl * 4, hipMemcpyDefault, st));
        HIPCHK(h, launch_shoot_gather(R.frames.as<float>(), h->stage.as<float>(), (int64_t)fl, N * c.O, T_, nullptr, gid, c.O, st));
        if (ol) {
            HIPCHK(h, hipMemcpyAsync(h->stage.p, node_type_onehot, ol * 4, hipMemcpyDefault, st));
            HIPCHK(h, launch_permute_rows(R.onehot.as<float>(), h->stage.as<float>(), gid, N, c.Fn - c.O, false, st));
        }
    } else {
        HIPCHK(h, hipMemcpyAsync(R.frames.p, frames, fl * 4, hipMemcpyDefault, st));
        if (ol) HIPCHK(h, hipMemcpyAsync(R.onehot.p, node_type_onehot, ol * 4, hipMemcpyDefault, st));
    }
    if (el && !part) HIPCHK(h, hipMemcpyAsync(R.ef_raw.p, ef_raw, el * 4, hipMemcpyDefault, st));   // (edge rows stay in the caller's order: the edge encoder reads them by edge_gid)
    HIPCHK(h, hipStreamSynchronize(st));
    R.T = T_;
    R.delta = std::move(delta);
    R.have = true;
    return MGN_OK;
} MGN_CATCH(h)

extern "C" int mgn_train_set_noise(mgn_handle* h, const float* stddev, const uint8_t* noisy, uint64_t seed) try {
    const char* who = "mgn_train_set_noise";
    if (!h) return MGN_E_ARG;
    if (int rc = datapoint_need(h, who, true, false)) return rc;
    TrainState::Trajectory& R = h->train->traj;
    const int64_t N = h->g.n_own;
    R.seed = seed;
    R.noise = false; R.some_nodes = false;
    if (!stddev) return MGN_OK;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, R.stddev.ensure((size_t)h->cfg.O * 4));
    HIPCHK(h, hipMemcpy(R.stddev.p, stddev, (size_t)h->cfg.O * 4, hipMemcpyDefault));
    if (noisy) {
        const bool by_gid = h->g.renumbered || h->cfg.nranks > 1;     // (a partition: `noisy` covers the mesh, the rank takes its own nodes' entries)
        const int64_t NG = h->cfg.nranks > 1 ? h->g.N : N;
        std::vector<uint8_t> in((size_t)NG), loc((size_t)N);
        HIPCHK(h, hipMemcpy(in.data(), noisy, (size_t)NG, hipMemcpyDefault));
        for (int64_t i = 0; i < N; ++i) loc[(size_t)i] = in[(size_t)(by_gid ? h->g.own_gid[(size_t)i] : i)] ? 1 : 0;
        HIPCHK(h, R.noisy.ensure((size_t)N));
        HIPCHK(h, hipMemcpy(R.noisy.p, loc.data(), (size_t)N, hipMemcpyHostToDevice));
        R.some_nodes = true;
    }
    R.noise = true;
    return MGN_OK;
} MGN_CATCH(h)

extern "C" int mgn_train_online_norms(mgn_handle* h, int32_t node_on, int32_t edge_on, int32_t out_on, double max_accumulations,
                                      float std_epsilon) try {
    const char* who = "mgn_train_online_norms";
    if (!h) return MGN_E_ARG;
    if (int rc = datapoint_need(h, who, false, false)) return rc;
    if (!(max_accumulations > 0.0) || !(std_epsilon > 0.f)) return fail(h, MGN_E_ARG, "%s: max_accumulations and std_epsilon must be positive", who);
    if (int rc = online_totals_ready(h)) return rc;
    if (int rc = datapoint_norms_ready(h)) return rc;
    TrainState& T = *h->train;
    const int32_t on[3] = {node_on, edge_on, out_on};
    for (int g = 0; g < 3; ++g) {
        TrainState::OnlineGroup& o = T.on[g];
        if (!on[g]) { o.online = false; o.dirty = false; continue; }      // (its entries of h->norms stay as they are)
        o = TrainState::OnlineGroup();
        o.online = true; o.max_acc = max_accumulations; o.eps = std_epsilon;
        HIPCHK(h, hipMemsetAsync(T.on_totals.as<double>() + online_off(h->cfg, g), 0, (size_t)2 * online_dim(h->cfg, g) * sizeof(double), h->stream));
    }
    return datapoint_norms_ready(h);
} MGN_CATCH(h)

extern "C" int mgn_train_norm_state(mgn_handle* h, int32_t group, int32_t write, double* sum, double* sum_squares, double* count_and_calls) try {
    const char* who = "mgn_train_norm_state";
    if (!h) return MGN_E_ARG;
    if (int rc = datapoint_need(h, who, false, false)) return rc;
    if (group < 0 || group > 2) return fail(h, MGN_E_ARG, "%s: group %d (0 node state columns, 1 edge, 2 output)", who, (int)group);
    if (!sum || !sum_squares || !count_and_calls) return fail(h, MGN_E_ARG, "%s: null argument", who);
    if (int rc = online_totals_ready(h)) return rc;
    TrainState::OnlineGroup& o = h->train->on[group];
    const int dim = online_dim(h->cfg, group);
    double* tot = h->train->on_totals.as<double>() + online_off(h->cfg, group);
    const hipStream_t st = h->stream;
    if (write) {
        if (!(count_and_calls[0] >= 0.0) || !(count_and_calls[1] >= 0.0)) return fail(h, MGN_E_ARG, "%s: negative count", who);
        HIPCHK(h, hipMemcpyAsync(tot, sum, (size_t)dim * sizeof(double), hipMemcpyHostToDevice, st));
        HIPCHK(h, hipMemcpyAsync(tot + dim, sum_squares, (size_t)dim * sizeof(double), hipMemcpyHostToDevice, st));
        HIPCHK(h, hipStreamSynchronize(st));
        o.count = count_and_calls[0]; o.calls = count_and_calls[1];
        o.dirty = true;
    } else {
        HIPCHK(h, hipMemcpyAsync(sum, tot, (size_t)dim * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(h, hipMemcpyAsync(sum_squares, tot + dim, (size_t)dim * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(h, hipStreamSynchronize(st));
        count_and_calls[0] = o.count; count_and_calls[1] = o.calls;
    }
    return MGN_OK;
} MGN_CATCH(h)

extern "C" int mgn_step_datapoint(mgn_handle* h, int32_t datapoint, int32_t accumulate, const int32_t* mask, int64_t nmask,
                                  int32_t mask_index_base, float* grads, size_t n_grads, float* loss) try {
    const char* who = "mgn_step_datapoint";
    if (!h) return MGN_E_ARG;
    if (!mask || !grads || !loss) return fail(h, MGN_E_ARG, "%s: null argument", who);
    if (int rc = datapoint_need(h, who, true, true)) return rc;
    if (datapoint < 0 || datapoint > h->train->traj.T - 2)
        return fail(h, MGN_E_ARG, "%s: datapoint %d outside [0, %d]", who, (int)datapoint, (int)h->train->traj.T - 2);
    if (nmask < 1) return fail(h, MGN_E_ARG, "%s: empty mask", who);
    if (mask_index_base != 0 && mask_index_base != 1) return fail(h, MGN_E_ARG, "%s: mask_index_base must be 0 or 1", who);
    const int64_t n_nodes = h->cfg.nranks > 1 ? h->g.N : h->g.n_own;      // (a partition takes the mask of the whole mesh)
    for (int64_t i = 0; i < nmask; ++i) {
        const int64_t n = (int64_t)mask[i] - mask_index_base;
        if (n < 0 || n >= n_nodes) return fail(h, MGN_E_ARG, "%s: mask entry %lld out of range", who, (long long)i);
    }
    if (int rc = train_prepare(h, who, n_grads, true)) return rc;       // (the last check: the collectives begin behind it)
    TrainJob J;
    J.kind = JOB_DATAPOINT;
    J.datapoint = datapoint; J.accumulate = accumulate != 0;
    J.mask = mask; J.nmask = nmask; J.mask_index_base = mask_index_base;
    J.loss = loss; J.grads = grads;
    return train_run(h, J);
} MGN_CATCH(h)

// step! on the block-diagonal FeatureGraph of B datapoints (the reference's Args.batchsize, src/MeshGraphNets.jl:39,224): B times the rows
// per launch, one weight-gradient pass, one set of launches.  B = 1 is mgn_step_datapoint itself.  B > 1 runs train_run on the cached
// companion of B copies (mgn_solve.cpp: companion_engine; no norms, no inference latents), whose inputs datapoints_stage assembles from
// this handle's trajectory; this handle's own training arena, mask cache and captured graphs are not touched.
extern "C" int mgn_step_datapoints(mgn_handle* h, const int32_t* datapoints, int32_t B, int32_t accumulate, const int32_t* mask, int64_t nmask,
                                   int32_t mask_index_base, float* grads, size_t n_grads, float* loss, float* losses) try {
    const char* who = "mgn_step_datapoints";
    static_assert(DATAPOINT_BATCH_MAX == MGN_DATAPOINT_BATCH_MAX, "the launch's table holds the ABI's largest batch");
    if (!h) return MGN_E_ARG;
    if (!datapoints || !mask || !grads || !loss) return fail(h, MGN_E_ARG, "%s: null argument", who);
    if (B < 1 || B > MGN_DATAPOINT_BATCH_MAX) return fail(h, MGN_E_ARG, "%s: B = %d outside [1, %d]", who, (int)B, MGN_DATAPOINT_BATCH_MAX);
    if (B == 1) {
        const int rc = mgn_step_datapoint(h, datapoints[0], accumulate, mask, nmask, mask_index_base, grads, n_grads, loss);
        if (!rc && losses) losses[0] = *loss;
        return rc;
    }
    if (int rc = datapoint_need(h, who, true, true)) return rc;
    if (h->cfg.nranks != 1) return fail(h, MGN_E_STATE, "%s with B > 1 drives one partition", who);
    const int32_t T_ = h->train->traj.T;
    for (int32_t b = 0; b < B; ++b)
        if (datapoints[b] < 0 || datapoints[b] > T_ - 2)
            return fail(h, MGN_E_ARG, "%s: datapoint %d (entry %d) outside [0, %d]", who, (int)datapoints[b], (int)b, (int)T_ - 2);
    if (nmask < 1) return fail(h, MGN_E_ARG, "%s: empty mask", who);
    if (mask_index_base != 0 && mask_index_base != 1) return fail(h, MGN_E_ARG, "%s: mask_index_base must be 0 or 1", who);
    const int64_t N = h->g.n_own, E = h->g.set[0].e_local;
    for (int64_t i = 0; i < nmask; ++i) {
        const int64_t n = (int64_t)mask[i] - mask_index_base;
        if (n < 0 || n >= N) return fail(h, MGN_E_ARG, "%s: mask entry %lld out of range", who, (long long)i);
    }
    if ((int64_t)B * N > INT32_MAX || (int64_t)B * E > INT32_MAX)
        return fail(h, MGN_E_ARG, "%s: %d copies of %lld nodes and %lld edges overflow int32 ids", who, (int)B, (long long)N, (long long)E);
    if (h->nsets != 1) return fail(h, MGN_E_UNSUPPORTED, "%s with B > 1 takes one edge set (the companion replicates one)", who);
    if (h->cfg.ln_dims == MGN_LN_ALL)
        return fail(h, MGN_E_UNSUPPORTED, "%s with B > 1 and ln_dims = MGN_LN_ALL: whole-array statistics would span the batch, a different model", who);
    if (int rc = need(h, true, true, false, true)) return rc;
    if (n_grads != h->params.size()) return fail(h, MGN_E_ARG, "%s: grads has %zu floats, model has %zu", who, n_grads, h->params.size());
    mgn_engine* c = nullptr;
    if (int rc = companion_engine(h, B, who, false, &c)) return rc;
    c->err.clear();
    if (int rc = train_prepare(c, who, n_grads)) return fail(h, rc, "%s: companion: %s", who, c->err.c_str());
    TrainState::Batch& X = c->train->batch;
    if (h->g.renumbered && X.g2l.empty()) {
        X.g2l.assign((size_t)h->g.N, 0);
        for (int32_t i = 0; i < h->g.n_own; ++i) X.g2l[(size_t)h->g.own_gid[i]] = i;
    }
    TrainJob J;
    J.kind = JOB_DATAPOINTS;
    J.parent = h; J.datapoints = datapoints; J.B = B; J.accumulate = accumulate != 0; J.losses = losses;
    J.mask = mask; J.nmask = nmask; J.mask_index_base = mask_index_base;
    J.loss = loss; J.grads = grads;
    const int rc = train_run(c, J);
    if (rc && !c->err.empty()) return fail(h, rc, "%s: companion: %s", who, c->err.c_str());   // (an error of the parent's own stage stands as it is)
    return rc;
} MGN_CATCH(h)

extern "C" int mgn_datapoint_export(mgn_handle* h, int32_t datapoint, int32_t normalised, float* nf, float* ef, float* target) try {
    const char* who = "mgn_datapoint_export";
    if (!h) return MGN_E_ARG;
    if (int rc = datapoint_need(h, who, true, true)) return rc;
    TrainState::Trajectory& R = h->train->traj;
    if (datapoint < 0 || datapoint > R.T - 2) return fail(h, MGN_E_ARG, "%s: datapoint %d outside [0, %d]", who, (int)datapoint, (int)R.T - 2);
    const mgn_config& c = h->cfg;
    const int64_t N = h->g.n_own, E = h->g.set[0].e_local;
    const hipStream_t st = h->stream;
    if (int rc = normalised ? datapoint_norms(h, datapoint, false, st) : datapoint_norms_ready(h)) return rc;
    const size_t nfl = ((size_t)N * c.Fn + 63) / 64 * 64, tl = ((size_t)N * c.O + 63) / 64 * 64, el = (size_t)E * c.Fe;
    HIPCHK(h, h->stage.ensure((nfl + tl + el) * 4));
    float* snf = h->stage.as<float>();
    float* stg = snf + nfl;
    float* sef = stg + tl;
    // A partition assembles the rows it owns in the engine's order and the host puts them at their places in the caller's arrays of the
    // whole mesh (host arrays): rows of other ranks' nodes and edges are left as they are.  No collective.
    const bool part = c.nranks > 1;
    std::vector<float> hnf, htg, hef;
    if (nf || target) {
        DatapointArgs a = datapoint_args(h, datapoint, normalised != 0);
        a.nf = nf ? snf : nullptr; a.target = target ? stg : nullptr; a.scatter = part ? 0 : 1;
        if (!nf) a.ld = c.O;
        HIPCHK(h, launch_datapoint_assemble(a, st));
        if (part) {
            if (nf) { hnf.resize((size_t)N * c.Fn); HIPCHK(h, hipMemcpyAsync(hnf.data(), snf, hnf.size() * 4, hipMemcpyDeviceToHost, st)); }
            if (target) { htg.resize((size_t)N * c.O); HIPCHK(h, hipMemcpyAsync(htg.data(), stg, htg.size() * 4, hipMemcpyDeviceToHost, st)); }
        } else {
            if (nf) HIPCHK(h, hipMemcpyAsync(nf, snf, (size_t)N * c.Fn * 4, hipMemcpyDefault, st));
            if (target) HIPCHK(h, hipMemcpyAsync(target, stg, (size_t)N * c.O * 4, hipMemcpyDefault, st));
        }
    }
    if (ef && el) {
        const float* es = normalised && h->have_enorm ? h->norms.as<float>() + 2 * c.Fn : nullptr;
        HIPCHK(h, launch_affine_pad(R.ef_raw.as<float>(), c.Fe, nullptr, 0, es, es ? es + c.Fe : nullptr, sef, c.Fe, E, st));
        if (part) { hef.resize(el); HIPCHK(h, hipMemcpyAsync(hef.data(), sef, el * 4, hipMemcpyDeviceToHost, st)); }
        else HIPCHK(h, hipMemcpyAsync(ef, sef, el * 4, hipMemcpyDefault, st));
    }
    HIPCHK(h, hipStreamSynchronize(st));
    if (part) {
        const std::vector<int32_t>& own = h->g.own_gid;
        const std::vector<int64_t>& egid = h->g.set[0].edge_gid;
        for (int64_t i = 0; i < N && !hnf.empty(); ++i) memcpy(nf + (size_t)own[(size_t)i] * c.Fn, hnf.data() + (size_t)i * c.Fn, (size_t)c.Fn * 4);
        for (int64_t i = 0; i < N && !htg.empty(); ++i) memcpy(target + (size_t)own[(size_t)i] * c.O, htg.data() + (size_t)i * c.O, (size_t)c.O * 4);
        for (int64_t i = 0; i < E && !hef.empty(); ++i) memcpy(ef + (size_t)egid[(size_t)i] * c.Fe, hef.data() + (size_t)i * c.Fe, (size_t)c.Fe * 4);
    }
    return MGN_OK;
} MGN_CATCH(h)

int mgn::ode_vjp_run(mgn_handle* h, const float* x, const float* node_type_onehot, const float* ef_raw, const float* val_mask, const float* lambda,
                     float* dxdt, float* xbar, float* grads, size_t n_grads, bool partitions) {
    if (!x || !lambda || !xbar || !grads) return fail(h, MGN_E_ARG, "mgn_ode_vjp: null argument");
    if (int rc = train_prepare(h, "mgn_ode_vjp", n_grads, partitions)) return rc;
    const mgn_config& c = h->cfg;
    if (c.Fn < c.O) return fail(h, MGN_E_ARG, "mgn_ode_vjp: Fn < O");
    if ((c.Fn > c.O && !node_type_onehot) || (!ef_raw && h->g.set[0].E > 0)) return fail(h, MGN_E_ARG, "mgn_ode_vjp: null argument");
    TrainJob J;
    J.kind = JOB_RHS_VJP;
    J.x = x; J.onehot = node_type_onehot; J.ef = ef_raw; J.val_mask = val_mask; J.lambda = lambda;
    J.dxdt = dxdt; J.xbar = xbar; J.grads = grads;
    return train_run(h, J);
}

extern "C" int mgn_ode_vjp(mgn_handle* h, const float* x, const float* node_type_onehot, const float* ef_raw, const float* val_mask,
                           const float* lambda, float* dxdt, float* xbar, float* grads, size_t n_grads) try {
    if (!h) return MGN_E_ARG;
    return ode_vjp_run(h, x, node_type_onehot, ef_raw, val_mask, lambda, dxdt, xbar, grads, n_grads, false);
} MGN_CATCH(h)

namespace mgn {

int solver_prepare(mgn_engine* h, size_t n_grads) { return train_prepare(h, "mgn_solver_grad", n_grads); }
int solver_prepare_partitions(mgn_engine* h, const char* who, size_t n_grads) { return train_prepare(h, who, n_grads, true); }

namespace {

// The pieces of the reverse sweep: the statics staged once per call, the adjoint launches of a state (k_solver_adjoint: every loss term of
// state k, xbar folded in, the seed of the step before written), one VJP of the right-hand side through train_run, and the results at the
// end.
struct Sweep {
    mgn_engine* h;
    const SolverSweep& S;
    int64_t N = 0, n = 0, n_loss = 0;
    bool part = false;                         // a partition: N owned rows; the loss and the gradient fold over the ranks in finish()
    int O = 0, nb = 0;
    float* io = nullptr;                       // xbar [N][O] | lambda [N][O] | onehot [N][Fn-O] | val_mask [N], as TrainPass lays them out
    float* vm = nullptr;
    float gscale = 0.f;
    int64_t sidx = 0;                          // saves are visited last to first; save_step is non-decreasing
    int slot = 0;

    // is the last save not yet visited state k's?
    bool save_at(int64_t k) {
        while (S.theta && sidx >= 0 && S.theta[sidx] >= 0.0) --sidx;      // (a save interpolated inside a step: not a state's)
        return sidx >= 0 && S.save_step[sidx] == k;
    }

    Sweep(mgn_engine* h_, const SolverSweep& S_) : h(h_), S(S_) {}

    int begin() {
        const mgn_config& c = h->cfg;
        N = h->g.n_own; O = c.O; n = N * O;
        TrainJob J;                                // the statics, once per call
        J.kind = JOB_SWEEP_STEP;
        J.onehot = S.onehot; J.val_mask = S.val_mask; J.ef = S.ef_raw;
        TrainPass P(h, J);
        io = P.io();
        vm = S.val_mask ? io + (size_t)N * (O + c.Fn) : nullptr;
        if (int rc = P.stage_statics(nullptr)) return rc;
        HIPCHK(h, hipMemsetAsync(S.a, 0, (size_t)n * 4, h->stream));
        nb = solver_adjoint_blocks(N, O);
        part = c.nranks > 1;
        n_loss = part ? (int64_t)h->g.N * O : n;       // the divisor of the save term: the whole mesh's N O, not a partition's rows
        gscale = (float)(2.0 / ((double)S.n_saves * (double)(S.win_rows > 0 ? S.win_rows * O : n_loss)));
        sidx = S.n_saves - 1;
        return MGN_OK;
    }

    // every loss term of state k (one launch per save that ends there; the continuity seed rides on the first), xbar folded in by the
    // first launch, the seed `seed * a` of the step before written into the VJP's lambda slot by the last
    int adjoint(int64_t k, bool with_xbar, float seed) {
        for (bool first = true;; first = false) {
            SolverAdjArgs p{};
            p.a = S.a;
            p.xbar = (first && with_xbar) ? io : nullptr;
            p.inflow = S.inflow;
            const bool has_save = save_at(k);
            if (has_save) {
                p.xs = S.saves + (size_t)sidx * n; p.gt = S.gt + (size_t)sidx * n; p.ls = S.loss_scale; p.vm = vm; p.gscale = gscale;
                --sidx;
            }
            if (first && k == S.K && S.cont_target) { p.xend = S.xend; p.ct = S.cont_target; p.cw = S.cont_weight; }
            const bool more = save_at(k);
            p.lam = (!more && k > 0) ? io + n : nullptr;
            p.dt = seed; p.N = N; p.O = O;
            if (S.lacc) {          // mgn_shooting_grad: per-window continuity weights, partials added across the call
                ShootAdjArgs q{p.a, p.lam, p.xbar, p.inflow, p.xs, p.gt, p.ls, p.vm, p.gscale, p.xend, p.ct, S.cw_win, S.win_rows,
                               p.dt, N, O, (p.gt || p.ct) ? S.lacc : nullptr, S.lacc_ld, S.lscale};
                HIPCHK(h, launch_shoot_adjoint(q, h->stream));
                if (!more) return MGN_OK;
                continue;
            }
            if (p.gt || p.ct) p.part = S.part + (size_t)slot++ * 2 * nb;
            HIPCHK(h, launch_solver_adjoint(p, h->stream));
            if (!more) return MGN_OK;
        }
    }

    // one VJP of the right-hand side at x (device, engine order) with the seed already in io's lambda slot: xbar into io, the parameter
    // gradient into the double accumulator (first: assigned)
    int vjp(const float* x, bool first) {
        TrainJob J;
        J.kind = JOB_SWEEP_STEP;
        J.first = first && !S.lacc;       // (mgn_shooting_grad: every pass adds to the zeroed accumulator)
        J.x = x;
        J.val_mask = vm;
        J.gacc = S.gacc;
        return train_run(h, J);
    }

    int finish() {
        if (S.lacc) return MGN_OK;        // mgn_shooting_grad finalises once for all its passes
        hipStream_t st = h->stream;
        const int64_t P = (int64_t)h->params.size();
        float* G = h->train->grads.as<float>();
        if (!part) {
            if (S.K > 0) HIPCHK(h, launch_grad_finish(S.gacc, G, P, st));
            else HIPCHK(h, hipMemsetAsync(G, 0, (size_t)P * 4, st));
            HIPCHK(h, hipMemcpyAsync(S.grads, G, (size_t)P * 4, hipMemcpyDefault, st));
        }
        std::vector<double> lp((size_t)slot * 2 * nb);
        if (!lp.empty()) HIPCHK(h, hipMemcpyAsync(lp.data(), S.part, lp.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(h, hipStreamSynchronize(st));
        double se = 0.0, sa = 0.0;
        for (int i = 0; i < slot; ++i)
            for (int b = 0; b < nb; ++b) {
                se += lp[(size_t)i * 2 * nb + b];
                sa += lp[(size_t)i * 2 * nb + nb + b];
            }
        if (part) {
            // once per call: this rank's two loss sums (the save terms, the continuity term) and its double accumulator, as it stands,
            // are gathered and added over the ranks in ascending order in double; the gradient is rounded to fp32 there, once, as
            // launch_grad_finish rounds it on one partition.  The same bits on every rank, the same bits on every call.
            double head[2] = {se, sa};
            if (int rc = rank_fold_f64(h, head, 2, S.K > 0 ? S.gacc : nullptr, P, G)) return rc;
            se = head[0]; sa = head[1];
            HIPCHK(h, hipMemcpyAsync(S.grads, G, (size_t)P * 4, hipMemcpyDefault, st));
            HIPCHK(h, hipStreamSynchronize(st));
        }
        *S.loss = (float)(se / ((double)S.n_saves * (double)n_loss) + (double)S.cont_weight * sa);
        return MGN_OK;
    }
};

}  // namespace

// The reverse sweep of solver-based training (mgn_solver_grad*, mgn_shooting_grad), driven by the tableau (S.stages active stages s, S.b,
// S.A; Euler: s = 1; Tsit5: s = 6, b = A[7]): steps n = K-1 .. 0, stages i = s .. 1, one VJP per stage on its stored input z_{n,i}.  The seed of stage s is written
// by the adjoint launch of state n + 1 (h_n b_s lam); k_erk_stage_seed masks zbar_{i+1} into ybar_{i+1} and writes
// kbar_i = h_n (b_i lam + sum_{j>i} A[j][i] ybar_j) for i = s-1 .. 1, and before stage 1's VJP adds sum_{j>=2} ybar_j to lam; the adjoint
// launch of state n folds in ybar_1 and the loss terms of x_n.  One stage (Euler): no seed launch at all.  No host
// synchronisation until the end.
//
// Dense saves (S.theta): the saves interpolated inside step n, xhat_s = x_n + h_n sum_i b_i(theta_s) k_{n,i}, seed lam_n with sum ghat_s,
// kbar_{n,i} with h_n W_i (W_i = sum_s b_i(theta_s) ghat_s, i = 1 .. 6) and, k_{n,7} being the evaluation at z_{n+1,1} (FSAL),
// kbar_{n+1,1} with h_n W_7.  ghat_s needs forward values only, so one k_tsit5_dense_adjoint launch per TSIT5_DENSE_MAX saves of step n
// runs right before the VJP at z_{n+1,1} -- stage 1 of step n + 1, whose seed launch has just consumed that step's own sums, or for the
// last step one extra VJP at z_{K,1} before the sweep starts, its masked output folded into lam_K by the adjoint launch of state K.
int erk_sweep(mgn_engine* h, const SolverSweep& S) {
    const int sp = S.stages;
    if (sp < 1 || sp > 6 || !S.b || !S.A) return fail(h, MGN_E_STATE, "erk_sweep: %d stages", sp);
    if (S.theta && sp != 6) return fail(h, MGN_E_STATE, "erk_sweep: interpolated saves are Tsit5's dense output");
    Sweep W(h, S);
    if (int rc = W.begin()) return rc;
    // the interpolated saves of every step, ascending
    std::vector<std::vector<int32_t>> inner(S.theta ? (size_t)S.K : 0);
    for (int32_t s = 0; S.theta && s < S.n_saves; ++s)
        if (S.theta[s] >= 0.0) {
            if (S.save_step[s] < 0 || S.save_step[s] >= S.K || !S.dense || !S.zend || S.lacc) return fail(h, MGN_E_STATE, "erk_sweep: bad dense-save plan");
            inner[(size_t)S.save_step[s]].push_back(s);
        }
    auto has_inner = [&](int64_t k) { return k >= 0 && k < (int64_t)inner.size() && !inner[(size_t)k].empty(); };
    // the launches of step m's interpolated saves: S.dense <- its sums, the VJP's lambda slot (+)= h_m W_7
    auto dense = [&](int64_t m, bool kbar_add) -> int {
        const std::vector<int32_t>& sv = inner[(size_t)m];
        for (size_t j0 = 0; j0 < sv.size(); j0 += TSIT5_DENSE_MAX) {
            Tsit5DenseArgs p{};
            p.ns = (int32_t)std::min<size_t>(TSIT5_DENSE_MAX, sv.size() - j0);
            for (int j = 0; j < p.ns; ++j) {
                const int32_t s = sv[j0 + j];
                double b[7];
                if (mgn_tsit5_interp_weights(S.theta[s], b) != MGN_OK) return fail(h, MGN_E_STATE, "erk_sweep: theta = %g of save %d", S.theta[s], s);
                for (int i = 0; i < 7; ++i) p.b[j][i] = (float)b[i];
                p.xs[j] = S.saves + (size_t)s * W.n; p.gt[j] = S.gt + (size_t)s * W.n;
                p.part[j] = S.part + (size_t)W.slot++ * 2 * W.nb;
            }
            p.ls = S.loss_scale; p.vm = W.vm; p.gscale = W.gscale;
            p.w = S.dense; p.kbar = W.io + W.n; p.h = (float)S.h[m];
            p.accumulate = j0 > 0; p.kbar_add = kbar_add || j0 > 0;
            p.N = W.N; p.O = W.O; p.nblk = W.nb;
            HIPCHK(h, launch_tsit5_dense_adjoint(p, h->stream));
        }
        return MGN_OK;
    };
    auto seed6 = [&](int64_t k) { return k > 0 ? (float)(S.h[k - 1] * S.b[sp - 1]) : 0.f; };      // the last stage's seed: h b_s lam
    bool first = true;                          // no VJP has run yet (the first one assigns the gradient accumulator)
    if (has_inner(S.K - 1)) {
        if (int rc = dense(S.K - 1, false)) return rc;
        if (int rc = W.vjp(S.zend, true)) return rc;
        first = false;
    }
    if (int rc = W.adjoint(S.K, !first, seed6(S.K))) return rc;
    for (int64_t k = S.K - 1; k >= 0; --k) {
        const bool di = has_inner(k);
        for (int i = sp; i >= 1; --i) {
            if (i < sp || di) {                 // (stage s's seed h_k b_s lam is the adjoint launch's; with dense saves it takes h_k W_6)
                ErkSeedArgs p{};
                p.xbar = i < sp ? W.io : nullptr;
                p.inflow = S.inflow;
                p.ybar = S.ybar;
                p.a = S.a;
                p.kbar = W.io + W.n;
                p.cb = (float)(S.h[k] * S.b[i - 1]);
                for (int j = i + 1; j <= sp; ++j) p.ca[j - 1] = (float)(S.h[k] * S.A[j - 1][i - 1]);
                p.i = i;
                p.s = sp;
                p.N = W.N;
                p.O = W.O;
                if (di) { p.w = S.dense + (size_t)i * W.n; p.g = i == 1 ? S.dense : nullptr; p.hw = (float)S.h[k]; }
                HIPCHK(h, launch_erk_stage_seed(p, h->stream));
            }
            if (i == 1 && has_inner(k - 1))
                if (int rc = dense(k - 1, true)) return rc;
            if (int rc = W.vjp(S.steps[k] + (size_t)(i - 1) * W.n, first)) return rc;
            first = false;
        }
        if (int rc = W.adjoint(k, true, seed6(k))) return rc;
    }
    return W.finish();
}

}  // namespace mgn

// =====================================================================================================================================
// mgn_config.ln_dims = MGN_LN_ALL: LayerNorm statistics over the whole (rows x L) output of an MLP -- what Lux 0.5's LayerNorm(shape)
// computes when GraphNetCore leaves it at dims = Colon() (reference Project.toml:15,40; julia/spec_probe.jl tells).  Every LayerNorm
// then couples all nodes / all edges, so nothing of it can be fused into a tile kernel: per MLP one launch of the training-forward
// kernel with its own LayerNorm off (train.hip: k_mlp_fwd, weights in training order), one grid-wide statistics pass (double, fixed
// order), one apply pass (+ residual).  Correct first: fp32-MFMA kernels, un-factored first edge layer, no kept activations.
// Serves mgn_forward (the model call, reference src/solve.jl:200) and mgn_processor_steps.
// =====================================================================================================================================
namespace {

struct LnAll {
    mgn_engine* h;
    TrainState& T;
    hipStream_t st;
    float* A;
    const float* Wt;
    int L;
    int64_t N, E;
    int32_t nt_n, nt_e;
    const int32_t *snd, *rcv, *rowptr, *egid;
    size_t V, Ecur, Y, Hb, agg, stats, part, nf_raw, nf_pad, ef_raw, ef_pad, tmp, E0, Pn, Qn;
    float eps_in, eps_out;
    int64_t slots = 0;           // (sum, sum of squares) slots the last MLP launch left in `part` (TrainFwdArgs::STATS)
    bool factored = false;       // large launches: the first edge layer per NODE (P = v W1s, Q = v W1r; launch_lin2) as in the training step

    void attach() {               // the device pointers, once the arena and the index arrays are there (lnall_bind)
        A = T.la.as<float>();
        snd = h->es[0].d_snd.as<int32_t>(); rcv = h->es[0].d_rcv.as<int32_t>(); rowptr = h->es[0].d_rowptr.as<int32_t>();
        egid = T.la_idx.as<int32_t>();
    }
    // Y <- MLP(x) without LayerNorm / residual (launch units chained through Hb); `in`, w1sel: as TrainPass::run_fwd takes them
    hipError_t mlp(const TrainMlp& m, const TrainFwdArgs& in, float* yout, int w1sel = -1) {
        for (int bi = 0; bi < m.nblk; ++bi) {
            const bool last = bi == m.nblk - 1;
            TrainFwdArgs a;
            const int nin = fwd_unit(m, bi, in, w1sel, Wt, A + Hb, a);
            a.ln = 0;
            a.OUT = last ? yout : A + Hb;
            if (last && m.b[bi].ln) { a.STATS = reinterpret_cast<double*>(A + part); slots = train_fwd_stat_slots(L, in.ntiles); }
            if (hipError_t e = launch_mlp_fwd(L, nin, a, st)) return e;
        }
        return hipSuccess;
    }
    // LayerNorm over all rows x L values of y with the MLP's gamma / beta: lnout = LN(y), out = resid + LN(y)
    hipError_t ln(const TrainMlp& m, const float* y, int64_t rows, const float* resid, float* out, float* lnout) {
        const TrainBlock& b = m.b[m.nblk - 1];
        const int64_t n = rows * L;
        if (n <= 0) return hipSuccess;
        if (hipError_t e = launch_array_stats_final(reinterpret_cast<const double*>(A + part), slots, n, eps_in, eps_out, A + stats, st)) return e;
        return launch_ln_all_apply(y, A + stats, Wt + b.tabs + (size_t)T_GAMMA * L, Wt + b.tabs + (size_t)T_BETA * L, resid, out, lnout, n, L, st);
    }
    // the edge half's LayerNorm, residual and aggregation in one pass over the receiver CSR (every edge has an owned receiver on one partition)
    hipError_t ln_edges(const TrainMlp& m, const float* y, float* e) {
        const TrainBlock& b = m.b[m.nblk - 1];
        if (hipError_t er = launch_array_stats_final(reinterpret_cast<const double*>(A + part), slots, E * L, eps_in, eps_out, A + stats, st)) return er;
        return launch_ln_all_apply_segsum(y, A + stats, Wt + b.tabs + (size_t)T_GAMMA * L, Wt + b.tabs + (size_t)T_BETA * L, e, rowptr, A + agg,
                                          (int32_t)N, L, st);
    }
    // one processor step on V / Ecur (engine order, row-major [rows][L])
    int step(int k) {
        float *v = A + V, *e = A + Ecur, *y = A + Y;
        if (E > 0 && factored) {
            const TrainMlp& m = T.m_pe[0][k];
            Lin2Args p{};
            p.rows = N; p.ntiles = nt_n;
            p.X0 = v; p.W0 = Wt + m.b[0].W1[0]; p.W1 = Wt + m.b[0].W1[1];
            p.OUT0 = A + Pn; p.OUT1 = A + Qn;
            HIPCHK(h, launch_lin2(L, p, st));
            TrainFwdArgs in = fwd_inputs(E, nt_e, e);
            in.PRE[0] = A + Pn; in.preidx[0] = snd; in.PRE[1] = A + Qn; in.preidx[1] = rcv;
            HIPCHK(h, mlp(m, in, y, 2));                                     // (the e block of W1 per edge)
            HIPCHK(h, ln_edges(m, y, e));                                    // e <- e + LN(y), agg <- segmented sum of LN(y)
        } else if (E > 0) {
            HIPCHK(h, mlp(T.m_pe[0][k], fwd_inputs(E, nt_e, v, snd, v, rcv, e), y));
            HIPCHK(h, ln_edges(T.m_pe[0][k], y, e));
        } else {
            HIPCHK(h, launch_segment_sum(L, y, rowptr, nullptr, nullptr, A + agg, (int32_t)N, st));   // (no edges: zero aggregates)
        }
        HIPCHK(h, mlp(T.m_pn[k], fwd_inputs(N, nt_n, v, nullptr, A + agg), y));
        HIPCHK(h, ln(T.m_pn[k], y, N, v, v, nullptr));                       // v <- v + LN(MLP_v([v; agg]))
        return MGN_OK;
    }
};

int lnall_prepare(mgn_engine* h) {
    if (!h) return MGN_E_ARG;
    if (h->host_only) return fail(h, MGN_E_HIP, "host-only handle (MGN_DEVICE_NONE): no compute path; create the handle on a HIP device");
    if (!h->have_params) return fail(h, MGN_E_STATE, "mgn_set_params has not been called");
    if (!h->have_graph) return fail(h, MGN_E_STATE, "mgn_set_graph has not been called");
    if (!h->train) h->train = new (std::nothrow) TrainState();
    if (!h->train) return fail(h, MGN_E_OOM, "host allocation failed");
    TrainState& T = *h->train;
    if (!T.packed)
        if (int rc = pack_training_weights(h)) return rc;
    return MGN_OK;
}

LnAll lnall_layout(mgn_engine* h, bool with_inputs, size_t& floats) {
    TrainState& T = *h->train;
    const LocalGraph& g = h->g;
    const mgn_config& c = h->cfg;
    LnAll X{h, T, h->stream, nullptr, T.w.as<float>(), c.L, g.n_own, g.set[0].e_local, 0, 0, nullptr, nullptr, nullptr, nullptr};
    X.nt_n = (int32_t)((X.N + TILE - 1) / TILE);
    X.nt_e = (int32_t)((X.E + TILE - 1) / TILE);
    const size_t NL = (size_t)(X.N > 0 ? X.N : 1) * c.L, EL = (size_t)(X.E > 0 ? X.E : 1) * c.L, ML = NL > EL ? NL : EL;
    size_t off = 0;
    auto take = [&](size_t n) { const size_t o = off; off += (n + 63) / 64 * 64; return o; };
    X.V = take(NL); X.Ecur = take(EL); X.Y = take(ML); X.Hb = T.nblk > 1 ? take(ML) : 0; X.agg = take(NL);
    X.factored = env_int("MGN_TRAIN_FACTORED", !train_uses_coop(128, X.nt_e)) != 0 && X.E > 0;
    X.Pn = X.Qn = 0;
    if (X.factored) { X.Pn = take(NL); X.Qn = take(NL); }
    X.stats = take(64);
    X.part = take(std::max<size_t>((size_t)4 * array_stats_blocks(), (size_t)16 * (size_t)std::max(X.nt_n, X.nt_e)));   // 2 doubles per slot
    X.tmp = take(ML);                                   // caller order <-> engine order staging
    X.nf_raw = X.nf_pad = X.ef_raw = X.ef_pad = X.E0 = 0;
    if (with_inputs) {
        X.nf_raw = take((size_t)X.N * c.Fn); X.nf_pad = take(NL);
        X.ef_raw = take((size_t)(X.E > 0 ? X.E : 1) * c.Fe); X.ef_pad = take(EL);
        X.E0 = take(EL);                                // the encoded edges of a trajectory (lnall_rhs_dev: the edge encoder runs once)
    }
    X.eps_in = c.ln_mode == MGN_LN_STD_EPS ? 0.f : 1e-5f;
    X.eps_out = c.ln_mode == MGN_LN_STD_EPS ? 1e-5f : 0.f;
    floats = off;
    return X;
}

int lnall_bind(mgn_engine* h, LnAll& X, size_t floats) {
    TrainState& T = *h->train;
    const LocalGraph& g = h->g;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, T.la.ensure(floats * 4));
    if (!T.la_ready) {
        std::vector<int32_t> eg((size_t)(X.E > 0 ? X.E : 1), 0);
        for (int64_t i = 0; i < X.E; ++i) eg[(size_t)i] = (int32_t)g.set[0].edge_gid[(size_t)i];
        HIPCHK(h, T.la_idx.ensure(eg.size() * 4));
        HIPCHK(h, hipMemcpy(T.la_idx.p, eg.data(), eg.size() * 4, hipMemcpyHostToDevice));
        T.la_ready = true;
    }
    X.attach();
    return MGN_OK;
}

}  // namespace

namespace mgn {

int lnall_forward(mgn_engine* h, const float* nf, const float* ef, float* out) {
    if (int rc = lnall_prepare(h)) return rc;
    h->lnall_edges = false;                             // (the arena is shared with the resident right-hand side)
    const mgn_config& c = h->cfg;
    const LocalGraph& g = h->g;
    if (!nf || !out || (!ef && g.set[0].E > 0)) return fail(h, MGN_E_ARG, "mgn_forward: null argument");
    size_t floats = 0;
    LnAll X = lnall_layout(h, true, floats);
    if (int rc = lnall_bind(h, X, floats)) return rc;
    TrainState& T = X.T;
    float* A = X.A;
    hipStream_t st = X.st;
    const int L = c.L;
    const int32_t* ngid = h->d_own_gid.as<int32_t>();
    // node features: caller's rows -> engine rows, padded to L; edge features stay in the caller's order and are gathered by edge id
    HIPCHK(h, hipMemcpyAsync(A + X.tmp, nf, (size_t)X.N * c.Fn * 4, hipMemcpyDefault, st));
    HIPCHK(h, launch_permute_rows(A + X.nf_raw, A + X.tmp, ngid, X.N, c.Fn, false, st));
    HIPCHK(h, launch_affine_pad(A + X.nf_raw, c.Fn, nullptr, 0, nullptr, nullptr, A + X.nf_pad, L, X.N, st));
    if (X.E > 0) {
        HIPCHK(h, hipMemcpyAsync(A + X.ef_raw, ef, (size_t)g.set[0].E * c.Fe * 4, hipMemcpyDefault, st));
        HIPCHK(h, launch_affine_pad(A + X.ef_raw, c.Fe, nullptr, 0, nullptr, nullptr, A + X.ef_pad, L, g.set[0].E, st));
    }
    // encoders
    HIPCHK(h, X.mlp(T.m_en, fwd_inputs(X.N, X.nt_n, A + X.nf_pad), A + X.Y));
    HIPCHK(h, X.ln(T.m_en, A + X.Y, X.N, nullptr, A + X.V, nullptr));
    if (X.E > 0) {
        HIPCHK(h, X.mlp(T.m_ee[0], fwd_inputs(X.E, X.nt_e, A + X.ef_pad, X.egid), A + X.Y));
        HIPCHK(h, X.ln(T.m_ee[0], A + X.Y, X.E, nullptr, A + X.Ecur, nullptr));
    }
    for (int k = 0; k < c.mps; ++k)
        if (int rc = X.step(k)) return rc;
    // decoder (no LayerNorm): the first O columns of its output, back in the caller's row order
    HIPCHK(h, X.mlp(T.m_de, fwd_inputs(X.N, X.nt_n, A + X.V), A + X.Y));
    HIPCHK(h, launch_extract_cols(A + X.Y, L, c.O, nullptr, A + X.agg, X.N, st));
    HIPCHK(h, launch_permute_rows(A + X.tmp, A + X.agg, ngid, X.N, c.O, true, st));
    HIPCHK(h, hipMemcpyAsync(out, A + X.tmp, (size_t)X.N * c.O * 4, hipMemcpyDefault, st));
    HIPCHK(h, hipStreamSynchronize(st));
    return MGN_OK;
}

int lnall_processor_steps(mgn_engine* h, float* v, float* e, int32_t nsteps) {
    if (int rc = lnall_prepare(h)) return rc;
    h->lnall_edges = false;
    const mgn_config& c = h->cfg;
    const LocalGraph& g = h->g;
    if (!v || (!e && g.set[0].E > 0)) return fail(h, MGN_E_ARG, "mgn_processor_steps: null argument");
    if (nsteps < 0 || nsteps > c.mps) return fail(h, MGN_E_ARG, "mgn_processor_steps: nsteps out of range");
    size_t floats = 0;
    LnAll X = lnall_layout(h, false, floats);
    if (int rc = lnall_bind(h, X, floats)) return rc;
    float* A = X.A;
    hipStream_t st = X.st;
    const int L = c.L;
    const int32_t* ngid = h->d_own_gid.as<int32_t>();
    HIPCHK(h, hipMemcpyAsync(A + X.tmp, v, (size_t)X.N * L * 4, hipMemcpyDefault, st));
    HIPCHK(h, launch_permute_rows(A + X.V, A + X.tmp, ngid, X.N, L, false, st));
    if (X.E > 0) {
        HIPCHK(h, hipMemcpyAsync(A + X.tmp, e, (size_t)X.E * L * 4, hipMemcpyDefault, st));
        HIPCHK(h, launch_permute_rows(A + X.Ecur, A + X.tmp, X.egid, X.E, L, false, st));
    }
    for (int k = 0; k < nsteps; ++k)
        if (int rc = X.step(k)) return rc;
    HIPCHK(h, launch_permute_rows(A + X.tmp, A + X.V, ngid, X.N, L, true, st));
    HIPCHK(h, hipMemcpyAsync(v, A + X.tmp, (size_t)X.N * L * 4, hipMemcpyDefault, st));
    if (X.E > 0) {
        HIPCHK(h, hipStreamSynchronize(st));
        HIPCHK(h, launch_permute_rows(A + X.tmp, A + X.Ecur, X.egid, X.E, L, true, st));
        HIPCHK(h, hipMemcpyAsync(e, A + X.tmp, (size_t)X.E * L * 4, hipMemcpyDefault, st));
    }
    HIPCHK(h, hipStreamSynchronize(st));
    return MGN_OK;
}

// The right-hand side on resident inputs under ln_dims = MGN_LN_ALL -- what encode_impl + run_processor + decode_impl (mgn_api.cpp) are to
// the fused kernels: node inputs [state (srcA, in_wa columns) | static (d_nfB, in_wb columns)] and raw edge features as upload_inputs left
// them (caller's order with own_gid / edge_gid, or the engine's order), build_graph's normalisers, the model, inverse_data, val_mask;
// out [n_own][O] in the engine's order.  reuse_edges: the encoded edge latents of the trajectory are taken from the arena (static edge
// features, frozen e_norm: the edge encoder runs once per trajectory).  Launches only -- no host copy, no synchronisation -- once
// lnall_rhs_prepare has bound the arena, so the rollout driver can capture it.
int lnall_rhs_prepare(mgn_engine* h) {
    if (int rc = lnall_prepare(h)) return rc;
    size_t floats = 0;
    LnAll X = lnall_layout(h, true, floats);
    return lnall_bind(h, X, floats);
}

int lnall_rhs_dev(mgn_engine* h, const float* srcA, float* out, bool reuse_edges) {
    const mgn_config& c = h->cfg;
    size_t floats = 0;
    LnAll X = lnall_layout(h, true, floats);
    TrainState& T = X.T;
    if (!T.la.p || T.la.bytes < floats * 4 || !T.la_ready) return fail(h, MGN_E_STATE, "whole-array LayerNorm: the right-hand side was not prepared");
    X.attach();
    float* A = X.A;
    hipStream_t st = X.st;
    const int L = c.L;
    const float* nrm = h->norms.as<float>();
    const int32_t* ngid = h->in_local ? nullptr : h->d_own_gid.as<int32_t>();
    const float* ns = h->have_nnorm ? nrm : nullptr;
    // node inputs: [srcA | srcB] normalised and padded to L, rows in the engine's order
    float* padded = ngid ? A + X.tmp : A + X.nf_pad;
    HIPCHK(h, launch_affine_pad(srcA, h->in_wa, h->d_nfB.as<float>(), h->in_wb, ns, ns ? ns + c.Fn : nullptr, padded, L, X.N, st));
    if (ngid) HIPCHK(h, launch_permute_rows(A + X.nf_pad, A + X.tmp, ngid, X.N, L, false, st));
    HIPCHK(h, X.mlp(T.m_en, fwd_inputs(X.N, X.nt_n, A + X.nf_pad), A + X.Y));
    HIPCHK(h, X.ln(T.m_en, A + X.Y, X.N, nullptr, A + X.V, nullptr));
    if (X.E > 0) {
        if (!reuse_edges) {
            const float* es = h->have_enorm ? nrm + 2 * c.Fn : nullptr;
            HIPCHK(h, launch_affine_pad(h->es[0].d_ef.as<float>(), c.Fe, nullptr, 0, es, es ? es + c.Fe : nullptr, A + X.ef_pad, L, X.E, st));
            HIPCHK(h, X.mlp(T.m_ee[0], fwd_inputs(X.E, X.nt_e, A + X.ef_pad, h->in_local ? nullptr : X.egid), A + X.Y));
            HIPCHK(h, X.ln(T.m_ee[0], A + X.Y, X.E, nullptr, A + X.E0, nullptr));
        }
        HIPCHK(h, hipMemcpyAsync(A + X.Ecur, A + X.E0, (size_t)X.E * L * 4, hipMemcpyDeviceToDevice, st));
    }
    for (int k = 0; k < c.mps; ++k)
        if (int rc = X.step(k)) return rc;
    HIPCHK(h, X.mlp(T.m_de, fwd_inputs(X.N, X.nt_n, A + X.V), A + X.Y));
    const float* os = h->have_onorm ? nrm + 2 * c.Fn + 2 * c.Fe : nullptr;
    HIPCHK(h, launch_rhs_epilogue(A + X.Y, L, c.O, os, os ? os + c.O : nullptr, h->have_mask ? h->d_mask.as<float>() : nullptr,
                                  h->d_own_gid.as<int32_t>(), out, X.N, st));
    return MGN_OK;
}

}  // namespace mgn

// Pullback of mgn_forward == the model call `mgn.model(graph, ps, st)` at reference src/solve.jl:200 (what a ChainRulesCore.rrule of
// the Julia shim's model function returns to Zygote inside the pullback of ode_func_train, src/strategies.jl:183-195): given the
// cotangent ybar of the output, nfbar = ybar^T d out / d nf (all Fn columns) and grads = ybar^T d out / d ps.
int mgn::forward_vjp_run(mgn_handle* h, const float* nf, const float* ef, const float* ybar, float* out, float* nfbar, float* grads, size_t n_grads,
                         bool partitions) {
    if (!nf || !ybar || !nfbar || !grads) return fail(h, MGN_E_ARG, "mgn_forward_vjp: null argument");
    if (int rc = train_prepare(h, "mgn_forward_vjp", n_grads, partitions)) return rc;
    if (!ef && h->g.set[0].E > 0) return fail(h, MGN_E_ARG, "mgn_forward_vjp: null argument");
    TrainJob J;
    J.kind = JOB_FORWARD_VJP;
    J.nf = nf; J.ef = ef; J.lambda = ybar; J.out = out; J.nfbar = nfbar; J.grads = grads;
    return train_run(h, J);
}

extern "C" int mgn_forward_vjp(mgn_handle* h, const float* nf, const float* ef, const float* ybar, float* out, float* nfbar, float* grads,
                               size_t n_grads) try {
    if (!h) return MGN_E_ARG;
    return forward_vjp_run(h, nf, ef, ybar, out, nfbar, grads, n_grads, false);
} MGN_CATCH(h)

// Online-normaliser accumulation (GraphNetCore NormaliserOnline, used at reference src/MeshGraphNets.jl:92,193-199 and inside
// build_graph): per-feature sum and sum of squares of x [rows][dim], in double.
extern "C" int mgn_feature_stats(mgn_handle* h, const float* x, int64_t rows, int32_t dim, double* sum, double* sum_squares) try {
    if (!h) return MGN_E_ARG;
    if (int rc = need(h, false, false)) return rc;
    if (!x || !sum || !sum_squares || rows < 0 || dim < 1) return fail(h, MGN_E_ARG, "mgn_feature_stats: bad argument");
    for (int f = 0; f < dim; ++f) sum[f] = sum_squares[f] = 0.0;
    const int nb = stats_blocks(rows);
    if (nb == 0) return MGN_OK;
    const size_t xbytes = (size_t)rows * dim * 4, pbytes = (size_t)nb * 2 * dim * sizeof(double);
    HIPCHK(h, h->stage.ensure(xbytes + pbytes + 64));
    float* dx = h->stage.as<float>();
    double* dp = reinterpret_cast<double*>(reinterpret_cast<char*>(h->stage.p) + (xbytes + 63) / 64 * 64);
    HIPCHK(h, hipMemcpyAsync(dx, x, xbytes, hipMemcpyDefault, h->stream));       // host or device source
    HIPCHK(h, launch_col_stats(dx, rows, dim, dp, h->stream));
    std::vector<double> part((size_t)nb * 2 * dim);
    HIPCHK(h, hipMemcpyAsync(part.data(), dp, pbytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int b = 0; b < nb; ++b)
        for (int f = 0; f < dim; ++f) {
            sum[f] += part[((size_t)b * 2 + 0) * dim + f];
            sum_squares[f] += part[((size_t)b * 2 + 1) * dim + f];
        }
    return MGN_OK;
} MGN_CATCH(h)

// tests: which regime the training launches ran in (beside the family codes).  out[0 .. 11]: launches of launch_mlp_fwd,
// launch_mlp_bwd and launch_lin2 since the last reset, four counters each -- cooperative, four-tile streaming, eight-tile streaming, and how
// many of the three ran on fp16 pieces (process-wide; a replayed hipGraph launches nothing here).  out[12 .. 19]: the plan of h's training
// state after a step -- factored (set 0, set 1), gsets, need_gt, keep_steps, rows per block of the weight-gradient launch of the processor's
// node MLP and of its edge MLPs (set 0, set 1) -- or -1 each without one.  h may be null (counts only); reset != 0 zeroes the counts
// after reading them.  Returns 0.
extern "C" int mgn_debug_train_regime(mgn_handle* h, int reset, int32_t* out /* [20] */) {
    int cnt[12];
    train_regime_counts(cnt, reset != 0);
    if (!out) return 0;
    for (int i = 0; i < 12; ++i) out[i] = cnt[i];
    for (int i = 12; i < 20; ++i) out[i] = -1;
    if (h && h->train && h->train->graph_ready) {
        const TrainState& T = *h->train;
        out[12] = T.factored[0]; out[13] = T.factored[1]; out[14] = T.gsets; out[15] = T.need_gt; out[16] = T.keep_steps;
        out[17] = (int32_t)T.wg_rpb_node; out[18] = (int32_t)T.wg_rpb_edge[0]; out[19] = (int32_t)T.wg_rpb_edge[1];
    }
    return 0;
}
// tests / bench: how many processor steps of the training arena keep their activations (-1: no training arena yet)
extern "C" int mgn_debug_train_keep_steps(mgn_handle* h) { return (h && h->train && h->train->graph_ready) ? h->train->keep_steps : -1; }
