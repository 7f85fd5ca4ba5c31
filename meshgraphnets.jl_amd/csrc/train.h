// Kernel argument blocks and launch wrappers of the training step (mgn_step == GraphNetCore.step!, reference
// src/strategies.jl:418-422).  Internal; the public boundary is include/mgn_hip.h.
//
// All training tensors are ROW-MAJOR [rows][L] fp32 (rows padded to whole 32-row tiles by the allocator); inputs
// narrower than L (node / edge features, decoder output) are zero-padded to L so that every MLP of the model --
// encoders, processor MLPs, decoder -- runs through the same three MFMA kernels:
//   k_mlp_fwd   forward, keeps the post-ReLU hidden activations H1, H2 and the pre-LayerNorm output Y
//   k_mlp_bwd   LayerNorm / ReLU / Dense backward w.r.t. the activations (transposed weight chunks)
//   k_wgrad     dW = X^T G  (reduction over rows on the MFMA, deterministic per-block partials) + column sums of G
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mgn {

struct TrainFwdArgs {
    int64_t rows; int32_t ntiles;
    const float* X[3]; const int32_t* xidx[3];   // layer-1 input blocks; xidx[j] != null: row gather
    const float* W1[3]; const float* W2; const float* W3;   // L x L chunks, fragment order (streamed from L2)
    const float* tabs;                           // T_B1, T_B2, T_B3, T_GAMMA, T_BETA (fragment order)
    float* H1; float* H2; float* Y;              // kept for the backward (null: not stored -- first pass of recompute mode)
    const float* resid; float* OUT;              // OUT = (resid ? resid : 0) + (ln ? LayerNorm(Y) : Y)
    float* LNOUT;                                // optional: LayerNorm(Y) alone (the message e' that is aggregated)
    // round 6, streaming kernels (train_fwd_fused_agg): the aggregation of e' = LayerNorm(Y) over runs of equal receiver inside the launch instead
    // of LNOUT + a segmented-sum pass -- rows are receiver-sorted, a run that lies inside a 32-row tile goes to SEG_AGG[receiver] (plain rows), the
    // pieces of a run that crosses tile borders to SEG_CARRY rows 2 tile (the part that continues from the tile before) / 2 tile + 1 (the part
    // that continues into the next); launch_seg_fixup adds the pieces up and zeroes the nodes without edges.  SEG_RCV: the receiver of every row.
    const int32_t* SEG_RCV; float* SEG_AGG; float* SEG_CARRY;
    int32_t ln;
    // factored first layer (edge MLP on large meshes): layer-1 pre-activation += PRE[i][preidx[i] ? preidx[i][row] : row]
    // (P = v W1_sender and Q = v W1_receiver, computed once per NODE by launch_lin2)
    const float* PRE[2]; const int32_t* preidx[2];
    // whole-array LayerNorm (ln = 0 here): (sum, sum of squares) of this launch's valid part of Y per slot, in double -- slot = tile for the
    // streaming kernels, 4 tile + wave for the cooperative ones (train_fwd_stat_slots); launch_array_stats_final adds the slots in order
    double* STATS;
};

struct TrainBwdArgs {
    int64_t rows; int32_t ntiles;
    const float* G0; const float* G1; const int32_t* g1idx;   // upstream gradient = G0[row] (+ G1[g1idx[row]])
    const float* Y; const float* H2; const float* H1;
    const float* W3T; const float* W2T; const float* W1T[3];  // transposed chunks, fragment order; W1T[j] null: skip
    const float* tabs;                           // gamma in T_GAMMA
    int32_t ln;                                  // 1: row-wise LayerNorm pullback here; 2: the whole-array one -- gy = rden (gamma g - m1 - xhat m2) with
    const float* LNS; const float* LNM;          //    LNS = (mean, rden, kappa) of the forward and LNM = (m1, m2) of launch_lnall_bwd; 0: none
    float* GT; float* GXH;                       // ln: total upstream gradient and G * xhat (-> dbeta, dgamma by column sums)
    float* LNSUM;                                // ln == 1, non-null (streaming kernels, 8 tiles per block; train_bwd_ln_sums): [block][2][L] column sums of the block's rows of g (dbeta) and g * xhat (dgamma), reduced inside the kernel (DPP adds over a tile's 32 rows, the block's waves through LDS) -- GT / GXH are not written then
    float* GY; float* GZ2; float* GZ1;           // gradients at the three Dense outputs (-> weight / bias gradients)
    float* GX[3]; const float* GXadd[3];         // GX[j][row] = (GXadd[j] ? GXadd[j][row] : 0) + GZ1[row] * W1T[j]
};

hipError_t launch_mlp_fwd(int L, int nin, const TrainFwdArgs& a, hipStream_t s);
bool train_fwd_fused_agg(int L, int ntiles);   // the forward launch of this size takes SEG_* (eight-tile streaming kernels)
// agg[n] = 0 for a node without edges, the sum of its carry rows for a node whose run of edges crosses tile borders (others: written by the forward kernel)
hipError_t launch_seg_fixup(int L, const int32_t* rowptr, const float* carry, float* agg, int32_t n, hipStream_t s);
hipError_t launch_mlp_bwd(int L, int nin, const TrainBwdArgs& a, hipStream_t s);
// L = 128: a non-empty MLP launch of at most this many tiles per CU of train_size_cus() runs the cooperative kernels, a larger one the
// eight-tile streaming kernels.  The same boundary decides the factored first edge layer and the second stream (mgn_train.cpp: prepare_graph).
constexpr int TRAIN_COOP_TILES_PER_CU = 8;
bool train_uses_coop(int L, int ntiles);
int train_size_cus();                      // the CU count the size rules of the training step are scaled by: 256 on every device, or the test CU count (kernels.h: set_num_cus)
void train_regime_counts(int* out /* [12] */, bool reset);   // launches since the last reset: [launch_mlp_fwd, launch_mlp_bwd, launch_lin2][cooperative, 4-tile streaming, 8-tile streaming, on fp16 pieces]
int set_train_f16(int on);                 // 1 (default): streaming training kernels at L = 128 on two fp16 pieces / three products, 0: fp32 MFMA; returns the old value     // the cooperative 4-wave MLP kernels serve this launch size

// Two L x L products per row tile (the per-node halves of the factored first edge layer):
//   split  (X1 == null):  OUT0 = X0 W0,  OUT1 = X0 W1                     (P, Q of the forward)
//   merge  (X1 != null):  OUT0 = (ADD ? ADD : 0) + X0 W0 + X1 W1          (gradient w.r.t. v from the summed GZ1 rows)
struct Lin2Args {
    int64_t rows; int32_t ntiles;
    const float* X0; const float* X1;
    const float* W0; const float* W1;            // chunks in fragment order
    const float* ADD; float* OUT0; float* OUT1;
};
hipError_t launch_lin2(int L, const Lin2Args& a, hipStream_t s);
// out_r[n] = sum over the receiver range of src (rows contiguous), out_s[n] = sum over the sender range of src[perm[p]]
hipError_t launch_segment_sum_pair(int L, const float* src, const int32_t* rowptr_r, const int32_t* rowptr_s, const int32_t* perm_s,
                                   float* out_r, float* out_s, int32_t n, hipStream_t s);

// Weight gradients of one MLP in ONE launch (blockIdx.y = job):
//   dW[in][out] = sum_rows X[xidx ? xidx[row] : row][in] * G[row][out];   db[out] = sum_rows G[row][out]
// The row range is split over wgrad_blocks(rows) blocks: pw [nblocks][L][L], pb [nblocks][L] hold per-block partials.
// pw == null: column sums only (LayerNorm parameter gradients); pb == null: no column sums.
// A launch carries the jobs of one launch unit: dW3, dW2, up to three blocks of dW1 (a factored edge MLP: the e block and the two node
// blocks) and the two column-sum jobs of the LayerNorm parameters.
constexpr int WGRAD_MAX_JOBS = 7;
struct WgradJob { const float* X; const int32_t* xidx; const float* G; int64_t rows; float* pw; float* pb; };
bool train_bwd_ln_sums(int L, int ntiles);   // the backward launch of this size takes LNSUM (eight-tile streaming kernels)
// out[g][c] = sum of part[b][c] over the g-th of `groups` equal ranges of the nblocks blocks, in order (c < cols): the first level of the LNSUM reduction
hipError_t launch_colsum_groups(const float* part, int nblocks, int cols, int groups, float* out, hipStream_t s);
struct WgradBatch { int32_t njobs; int64_t rows_per_block; WgradJob job[WGRAD_MAX_JOBS]; };
int wgrad_blocks(int64_t rows);
int64_t wgrad_rows_per_block(int64_t launch_rows);   // rows per block of a weight-gradient launch sized for launch_rows
int wgrad_blocks_of_job(int64_t launch_rows, int64_t job_rows);   // blocks of a launch sized for launch_rows that touch a job with fewer rows
// one L x L chunk of the inference layouts, from rows [kbase, kbase + L) of the matrix at params + src (leading dimension ldw).
// kind 0: fp32, three copies at wfrag + off (fragment order, t-major at + L L, 16x16x4 order at + 2 L L when L = 128);
// kind 1 / 2: the three exact bf16 pieces (hi, mid, lo; 16 384 each) at wsp + off in the 32x32x16 / 16x16x32 fragment order;
// kind 3: one bf16 copy at wbf + off (bf16 storage mode);
// kind 4: the two fp16 pieces (hi, lo; 16 384 each) of the chunk times `scale` (a power of two) at wsp + off, 32x32x16 fragment order
// (split_common.hpp); kind 5: the same in the 16x16x32 fragment order.  The host functions of mgn_api.cpp with the same names are the specification.
struct WPackJob { int kind; long long off, src; int ldw, kbase; float scale; };
hipError_t launch_pack_weights(int L, const WPackJob* jobs, int njobs, const float* params, float* wfrag, uint16_t* wsp, uint16_t* wbf, hipStream_t s);
// one packed copy of the training weights: kind 0 = an L x L chunk in fragment order + its t-major copy at + L * L, from rows [r0, r0 + nr)
// x cols [0, nc) of the matrix at params + src (leading dimension ldw; src < 0: the identity), zero-padded, transposed on request;
// kind 1 = the T_COUNT * L table floats of one launch unit, built from the parameter vector as tabs[src] describes them
struct PackJob { long long off, src; int ldw, r0, nr, nc, transpose, kind; float scale; };   // scale > 0 (L = 128): + the chunk's two fp16 pieces at off + 2 L L (32x32x16 fragment order: hi, lo), times the power of two that puts its largest entry into [2^14, 2^15) (taken on the device), and the inverse of that power at off + 3 L L
// The tables of one launch unit: rows T_B1 .. T_BETA hold the first cnt[t] floats at params + src[t] (src < 0: none) in pack_tab's
// order, zero behind them (an identity slot's bias, the decoder's O-wide last bias, no LayerNorm); T_BQ stays zero; T_LN holds
// (eps_in, eps_out).  Like the chunk list it depends on the configuration alone, never on the parameter values.
struct PackTab { long long src[5]; int cnt[5]; float eps_in, eps_out; };
hipError_t launch_pack_train(int L, const PackJob* jobs, int njobs, const float* params, const PackTab* tabs, unsigned* jobmax /* [njobs] scratch */, float* out, hipStream_t s);
// Optimisers.Adam on n floats, every operation rounded once in fp32 (mgn_hip.h: mgn_adam_update): c1, c2 = (float)(1 - beta_t)
#pragma GCC visibility push(hidden)   // (new host functions stay out of the library's dynamic symbols)
hipError_t launch_adam(float* p, float* m, float* v, const float* g, int64_t n, float eta, float b1, float b2, float eps, float c1, float c2,
                       hipStream_t s);
#pragma GCC visibility pop
hipError_t launch_wgrad(int L, WgradBatch wb, int64_t rows, hipStream_t s);
// out[r * cols + c] = sum_b partial[b * block_stride + r * ld + c]   (fixed order: bitwise reproducible), one job per blockIdx.y
constexpr int REDUCE_MAX_JOBS = 10;   // one launch unit: five weight blocks, three biases, dgamma and dbeta
struct ReduceJob { const float* partial; int32_t nblocks; int64_t block_stride; int32_t nrows, cols, ld; float* out; };
struct ReduceBatch { int32_t njobs; ReduceJob job[REDUCE_MAX_JOBS]; };
hipError_t launch_reduce_partials(const ReduceBatch& rb, hipStream_t s);
// out[n] = (add ? add[n] : 0) + sum_{p in [rowptr[n], rowptr[n+1])} src[perm ? perm[p] : p]   (rows of L floats)
hipError_t launch_segment_sum(int L, const float* src, const int32_t* rowptr, const int32_t* perm, const float* add, float* out,
                              int32_t n, hipStream_t s);
// out[n] = add[n] + sum_{p in A-range(n)} srcA[p] + sum_{p in B-range(n)} srcB[permB[p]]   (add may alias out)
hipError_t launch_segment_sum2(int L, const float* srcA, const int32_t* rowptrA, const float* srcB, const int32_t* rowptrB, const int32_t* permB,
                               const float* add, float* out, int32_t n, hipStream_t s);
// dst [rows][L] = [ (srcA | srcB)[rows][wa + wb] * scale + shift | 0 ]   (srcB may be null with wb = 0; scale null: identity)
hipError_t launch_affine_pad(const float* srcA, int wa, const float* srcB, int wb, const float* scale, const float* shift, float* dst, int L,
                             int64_t rows, hipStream_t s);
// the same with a row gather: dst row r <- source row gid[r] (gid null: row r)
hipError_t launch_affine_pad_gather(const float* srcA, int wa, const float* srcB, int wb, const float* scale, const float* shift, const int32_t* gid,
                                    float* dst, int L, int64_t rows, hipStream_t s);
// whole-array LayerNorm (mgn_config.ln_dims = MGN_LN_ALL): stats = (mean, 1 / (sqrt(var + eps_in) + eps_out), kappa) over the n values of x
// (double accumulation, fixed order; partial: 2 * array_stats_blocks() doubles), then t = (y - mean) * rden * gamma + beta
int array_stats_blocks();
int train_fwd_stat_slots(int L, int ntiles);     // slots a launch_mlp_fwd with TrainFwdArgs::STATS writes (2 doubles each)
hipError_t launch_array_stats_final(const double* partial, int64_t slots, int64_t n, float eps_in, float eps_out, float* stats, hipStream_t s);
hipError_t launch_array_stats(const float* x, int64_t n, double* partial, float eps_in, float eps_out, float* stats, hipStream_t s);
hipError_t launch_ln_all_apply(const float* y, const float* stats, const float* gamma, const float* beta, const float* resid, float* out,
                               float* lnout, int64_t n, int L, hipStream_t s);
// one pass over the receiver CSR: t = LN_all(y[p]); e[p] += t; agg[n] = sum of t over the edges node n receives (edge order)
hipError_t launch_ln_all_apply_segsum(const float* y, const float* stats, const float* gamma, const float* beta, float* e, const int32_t* rowptr,
                                      float* agg, int32_t n, int L, hipStream_t s);
// epilogue of a right-hand side: out [N][O] = (Y[:, 0:O] os + osh) .* mask[gid ? gid[row] : row]   (os / mask / gid may be null)
hipError_t launch_rhs_epilogue(const float* Y, int L, int O, const float* os, const float* osh, const float* mask, const int32_t* gid, float* out,
                               int64_t N, hipStream_t s);
// reverse pass of the whole-array LayerNorm of one MLP: dgamma, dbeta (L floats each, written into the gradient vector) and m = (m1, m2)
// (2 floats) for G = G0[row] (+ G1[g1idx ? g1idx[row] : row]); the MLP backward kernel then maps G to rden (gamma G - m1 - xhat m2) as it
// loads it (TrainBwdArgs::ln = 2).  partial: 2 * 128 * lnall_bwd_blocks() doubles; stats: (mean, rden, kappa) of the forward
int lnall_bwd_blocks();
hipError_t launch_lnall_bwd(const float* G0, const float* G1, const int32_t* g1idx, const float* Y, const float* stats, const float* gamma,
                            int64_t rows, int L, double* partial, float* m, float* dgamma, float* dbeta, hipStream_t s);
// node rows between the caller's order and the engine's (a renumbered graph: graph_host.h): gather dst[i] = src[gid[i]], scatter dst[gid[i]] = src[i]
hipError_t launch_permute_rows(float* dst, const float* src, const int32_t* gid, int64_t rows, int width, bool scatter, hipStream_t s);
// seed of the RHS VJP (mgn_ode_vjp): G[n][o] = lambda[n][o] * val_mask[n] * os[o]; optionally dxdt = (Y * os + osh) .* val_mask
hipError_t launch_vjp_seed(const float* Y, int L, int O, const float* lambda, const float* vm, const float* os, const float* osh, float* G,
                           float* dxdt, int64_t N, hipStream_t s);
// dst [N][O] = src[N][L][:, 0:O] .* scale
hipError_t launch_extract_cols(const float* src, int L, int O, const float* scale, float* dst, int64_t N, hipStream_t s);
// column statistics for the online normalisers: partial[b][0][f] = sum over block b's rows of x[r][f], partial[b][1][f] = sum of
// squares, in double, fixed order inside a block (stats_blocks(rows) blocks of STATS_ROWS rows; the caller adds the blocks in order)
constexpr int STATS_ROWS = 2048;
int stats_blocks(int64_t rows);
hipError_t launch_col_stats(const float* x, int64_t rows, int dim, double* partial, hipStream_t s);
// mgn_step_datapoint (reference src/strategies.jl:395-416, init_train_step of the derivative strategies): datapoint t of a resident
// trajectory, rows in the engine's order (gid[r]: the caller's id of row r, null: r).  Per state column o < O of row r:
//   cur = frame_t + stddev[o] z(seed, t, gid[r], o) where noisy[r] (stddev null: no noise; noisy null: every row); z: the generator of
//         k_randn_rows on the trajectory as a [T N][O] array;   d = (frame_{t+1} - cur) / delta;   target = (d - osh) / os
//   (nrm_o = [os | osh], null: target = d), IEEE fp32 operations one by one.
//   nf [N][ld] = [ [cur | onehot] * scale + shift | 0 ]  (nrm_n = [scale | shift] over Fn columns, null: as they are; k_affine_pad's expression)
// scatter: rows of nf / target go to gid[r] (the caller's order: exports).  raw_cur / raw_d [N][O] (null: not written): cur and d in
// the CALLER's order, what the online normalisers accumulate.  nf / target may be null.
// A partition (mgn_step_datapoint at nranks > 1) holds the N rows it owns, gid[r] is a node id of the whole mesh: Nkey, the rows of
// the noise generator's [T Nkey][O] array, is the mesh's node count (the noise of a node does not depend on the partition), and with
// raw_local the raw rows stay in the engine's order (raw_cur / raw_d have N rows, not Nkey).
struct DatapointArgs {
    const float* cur; const float* nxt; const float* onehot;
    const int32_t* gid; const uint8_t* noisy; const float* stddev;
    const float* nrm_n; const float* nrm_o;
    float* nf; float* target; float* raw_cur; float* raw_d;
    int64_t N, Nkey; int32_t O, Fn, ld, t, scatter, raw_local;
    float delta; uint64_t seed;
};
hipError_t launch_datapoint_assemble(const DatapointArgs& a, hipStream_t s);
// mgn_step_datapoints: B <= DATAPOINT_BATCH_MAX datapoints of the resident trajectory (one partition) as one block-diagonal FeatureGraph.
// Row r of the B N destination rows is copy w = r / N, engine row n = r mod N of datapoint t[w] (frames [T][N][O]; delta[w] its time
// step); per element the operations, the noise key (seed, t[w] N + gid[n], o) and the gid / noisy handling of launch_datapoint_assemble:
// nf [B N][ld] and target [B N][O] are the single launch's rows, copy after copy.  The table travels by value with the launch.
constexpr int DATAPOINT_BATCH_MAX = 64;
struct DatapointBatchArgs {
    const float* frames; const float* onehot;
    const int32_t* gid; const uint8_t* noisy; const float* stddev;
    const float* nrm_n; const float* nrm_o;
    float* nf; float* target;
    int64_t N; int32_t B, O, Fn, ld;
    uint64_t seed;
    int32_t t[DATAPOINT_BATCH_MAX]; float delta[DATAPOINT_BATCH_MAX];
};
#pragma GCC visibility push(hidden)   // (new host functions stay out of the library's dynamic symbols)
hipError_t launch_datapoints_assemble(const DatapointBatchArgs& a, hipStream_t s);
// dst [B E][L]: row w E + j = [ src[egid ? egid[j] : j][0:Fe] * scale + shift | 0 ] for every copy w (launch_affine_pad's expression, each
// row formed once): the trajectory's edge features, kept in the caller's order, in the engine's edge order of every copy
hipError_t launch_datapoints_edges(const float* src, int Fe, const float* scale, const float* shift, const int64_t* egid, float* dst, int L,
                                   int64_t E, int B, hipStream_t s);
// launch_loss over B copies of N rows with the mask listed once (entries of one copy): G[n + w N][o] += 2 (out - target) / (B nmask);
// partial [B][loss_blocks(nmask)] doubles in fixed slots; then one fold launch: out[w] = loss of copy w (its blocks added in order, over
// nmask), out[B] = the mean of the B, formed in double, each rounded once.  Bitwise repeatable where no mask entry repeats.
hipError_t launch_loss_batch(const float* Y, int L, const float* target, int O, const int32_t* mask, int64_t nmask, int64_t N, int B,
                             int32_t index_base, float* G, double* partial, float* out, hipStream_t s);
#pragma GCC visibility pop
// The online normalisers' maps from device-resident double totals [sum (dim) | sum of squares (dim)], one group each for the node state
// columns, the edge features and the output.  add: totals += this call's sums first -- `partial` (launch_col_stats' nb blocks, added in
// block order from zero: mgn_feature_stats' result) or, partial null, call_sums [2][dim] formed that way earlier.  write: scale / shift
// from the totals over `count` rows: mean and std in double, rounded to float, std = max(std, eps); scale = 1 / std, shift = -mean scale,
// or with `inverse` scale = std, shift = mean.  dim = 0: nothing.
// pstride: doubles from one block of `partial` to the next (0: 2 dim, launch_col_stats' layout).  A partitioned mesh adds the ranks'
// sums this way -- block b is rank b's [sum | sum of squares] inside the allgathered rows, nb = nranks: ascending rank order.
struct NormGroupArgs {
    const double* partial; const double* call_sums; double* totals; float* scale; float* shift;
    double count; float eps; int32_t nb, dim, add, write, inverse, pstride;
};
struct NormsFromTotalsArgs { NormGroupArgs g[3]; };
hipError_t launch_norms_from_totals(const NormsFromTotalsArgs& a, hipStream_t s);
// masked MSE: loss_partial[b] = sum over this block's mask entries of sum_o (out - target)^2;
// G[n][o] += 2 (out[n][o] - target[n][o]) / divisor   (G [N][L] zeroed by the caller; out = first O columns of Y; divisor = nmask, or on
// a partition, which lists only the entries it owns, the length of the whole mask)
int loss_blocks(int64_t nmask);
hipError_t launch_loss(const float* Y, int L, const float* target, int O, const int32_t* mask, int64_t nmask, int64_t divisor, int32_t index_base,
                       float* G, double* loss_partial, hipStream_t s);

// mgn_step on a partitioned mesh (nranks > 1): rows of L fp32 between the node arrays and the exchange buffers, and the finish.
//   pack        dst[r] = src[idx[r]]: the owned boundary rows in send-index order (peer-major), contiguous
//   unpack      halo_rows[r] = recv[r]: the halo rows are one block behind the owned rows, in the receive buffer's order
//   accumulate  g[row[b]] += recv[pos[p]], p in [ptr[b], ptr[b + 1]) in order: the halo rows' gradients arriving at their owner (a CSR
//               over the owned rows that some peer lists, positions ascending: own term, then peers by rank, then list order)
hipError_t launch_halo_pack(int L, const float* src, const int32_t* idx, float* dst, int64_t rows, hipStream_t s);
hipError_t launch_halo_unpack(int L, const float* recv, float* halo_rows, int64_t rows, hipStream_t s);
hipError_t launch_halo_accumulate(int L, const float* recv, const int32_t* row, const int32_t* ptr, const int32_t* pos, float* g, int32_t n,
                                  hipStream_t s);
// One rank's contribution to the finish: RANK_SUM_HEAD floats (the loss numerator as one double, the rest unused), then the n gradient
// floats zero-padded to a multiple of four -- rank_sum_stride(n) floats.  launch_loss_numerator adds the rank's loss partials into the
// head; launch_rank_sum adds all [nranks][stride] over the ranks in ascending order, in double: out [n] floats, loss[0] the numerator.
constexpr int RANK_SUM_HEAD = 4;
int64_t rank_sum_stride(int64_t n);
hipError_t launch_loss_numerator(const double* partial, int nb, double* out, hipStream_t s);
hipError_t launch_rank_sum(const float* all, int nranks, int64_t n, float* out, double* loss, hipStream_t s);
// The finish in double (solver-based training and rollout evaluation on a partitioned mesh): one rank's part is nhead sums (loss partials,
// evaluation sums), then n entries of a double accumulator, padded to rank_sum_f64_stride(nhead, n) doubles.  launch_rank_sum_f64 adds
// all [nranks][stride] over the ranks in ascending order, in double: head [nhead] doubles, out [n] floats (each rounded once).
#pragma GCC visibility push(hidden)   // (new host functions stay out of the library's dynamic symbols)
int64_t rank_sum_f64_stride(int64_t nhead, int64_t n);
hipError_t launch_rank_sum_f64(const double* all, int nranks, int64_t nhead, int64_t n, double* head, float* out, hipStream_t s);
// The fold of a replica group (mgn_group_step_datapoints): all [P][replica_fold_stride(n)] floats, replica k's gradient of its share of
// the minibatch (n floats, the row padded to a multiple of four so that every row starts on 16 bytes; the padding is never read).
//   out[i] = (float) s_P,   s_0 = +0.0,   s_{k+1} = active k ? s_k + w[k] * (double) all[k][i] : s_k      (k ascending)
// with every product and every sum rounded once in double and none contracted, so a float64 replay of "multiply, then add" gives the
// same bits.  w (by value, P <= REPLICA_FOLD_MAX) holds B_k / B; bit k of `active` says that replica k had a share: neither the row
// nor the weight of an idle replica is read.  No atomics; every replica runs it on the same gathered bytes.
constexpr int REPLICA_FOLD_MAX = 64;
struct ReplicaFoldW { double w[REPLICA_FOLD_MAX]; };
int64_t replica_fold_stride(int64_t n);
hipError_t launch_replica_fold(const float* all, int P, int64_t n, const ReplicaFoldW& w, uint64_t active, float* out, hipStream_t s);
#pragma GCC visibility pop

// solver-based training (mgn_solver_grad*, mgn_shooting_grad), state k of the reverse sweep (erk_sweep), per element of the [N][O] state:
//   a <- a + (xbar ? (inflow[n] ? 0 : xbar) : 0) + (gt ? -gscale ls[o]^2 (gt - xs) vm[n] : 0) + (ct ? cw sign(xend - ct) : 0);  lam <- dt a
// (dt: the seed factor of the last stage of the step before, h_{k-1} b_s; Euler: its dt)
// part (may be null): [2][solver_adjoint_blocks] doubles -- per block the sum of (ls (gt - xs))^2 vm, then of |xend - ct|
struct SolverAdjArgs {
    float* a; float* lam; const float* xbar; const uint8_t* inflow;
    const float* xs; const float* gt; const float* ls; const float* vm; float gscale;
    const float* xend; const float* ct; float cw;
    float dt; int64_t N; int32_t O;
    double* part;
};
int solver_adjoint_blocks(int64_t N, int O);
hipError_t launch_solver_adjoint(const SolverAdjArgs& p, hipStream_t s);
// solver-based training with an explicit Runge-Kutta tableau of s <= 6 active stages (mgn_solver_grad: s = 1, no launch; mgn_solver_grad_tsit5: s = 6; mgn_solver_grad_erk),
// stage i (1 .. s - 1) of the reverse pass of one step, per element of the [N][O] state, before the VJP of stage i:
//   ybar_{i+1} <- inflow[n] ? 0 : xbar  (the VJP of stage i + 1 just finished);   kbar <- cb lam + sum_{i<j<=s} ca[j - 1] ybar_j
//   (cb = h b[i], ca[j - 1] = h A[j][i]);   i = 1: lam <- lam + sum_{j=2..s} ybar_j as well.   ybar: [5][N][O], ybar_j at j - 2.
// A stage j whose coefficient is exactly 0 is left out of kbar without its ybar being read (i = 1 reads it for the sum); no slot of a
// stage beyond s is read.
// Dense saves (Tsit5; a step with interpolated saves, below): w (null: none) is the step's weighted sum W_i, added as kbar += hw w; g
// (i = 1 only, null: none) the sum of the interpolated saves' seeds, added to lam with the ybar.  i = s with xbar null is
// kbar <- cb lam (+ hw w), what the adjoint launch of the state after the step wrote.
struct ErkSeedArgs {
    const float* xbar; const uint8_t* inflow; float* ybar; float* a; float* kbar;
    float cb; float ca[6];
    int32_t i, s; int64_t N; int32_t O;
    const float* w; const float* g; float hw;
};
hipError_t launch_erk_stage_seed(const ErkSeedArgs& p, hipStream_t s);
// mgn_solver_grad_tsit5 with MGN_TSIT5_DENSE_SAVES: the loss terms of ns <= TSIT5_DENSE_MAX saves interpolated inside one accepted step,
// xs[s] = x_n + h sum_i b[s][i - 1] k_{n,i}, per element of the [N][O] state.  With ghat_s = -gscale ls[o]^2 (gt[s] - xs[s]) vm[n]:
//   w[0] (+)= sum_s ghat_s;   w[i] (+)= sum_s b[s][i - 1] ghat_s, i = 1 .. 6   (w: [7][N][O]; accumulate: added to what is there);
//   kbar (+)= h sum_s b[s][6] ghat_s   (the seed of the VJP at z_{n+1,1}, whose output is k_{n,7}; kbar_add: added to what is there)
// part[s]: [2][nblk] doubles as k_solver_adjoint leaves them, nblk = solver_adjoint_blocks(N, O) -- per block the sum of
// (ls (gt[s] - xs[s]))^2 vm, the rest zero.  Every element is owned by one thread and the saves are taken in order: no atomics.
constexpr int TSIT5_DENSE_MAX = 4;
struct Tsit5DenseArgs {
    const float* xs[TSIT5_DENSE_MAX]; const float* gt[TSIT5_DENSE_MAX]; double* part[TSIT5_DENSE_MAX];
    float b[TSIT5_DENSE_MAX][7];
    int32_t ns;
    const float* ls; const float* vm; float gscale;
    float* w; float* kbar; float h;
    int32_t accumulate, kbar_add;
    int64_t N; int32_t O; int32_t nblk;
};
hipError_t launch_tsit5_dense_adjoint(const Tsit5DenseArgs& p, hipStream_t s);
// mgn_shooting_grad: the state holds B windows of N rows each (row r is window r / N's row r mod N).
// The windowed adjoint step: k_solver_adjoint per element with the continuity weight of the row's window (cw_win[n / win_rows]: 0 for a
// window with no successor), and its loss terms ADDED to running per-block partials acc[0][b] (mse times lscale = 1 / (n_saves N O) of the
// group) and acc[ld + b] (cw_w |xend - ct|): the same block slot in every launch of a call, so the sums stay in a fixed order.
struct ShootAdjArgs {
    float* a; float* lam; const float* xbar; const uint8_t* inflow;
    const float* xs; const float* gt; const float* ls; const float* vm; float gscale;
    const float* xend; const float* ct; const float* cw_win; int64_t win_rows;
    float dt; int64_t N; int32_t O;
    double* acc; int32_t ld; double lscale;
};
hipError_t launch_shoot_adjoint(const ShootAdjArgs& p, hipStream_t s);
// the batched inflow overwrite: x[r][:] = frames[ftab[r / N]][r mod N][:] where mask[r mod N]   (rows = B N; frames [n_frames][N][O])
hipError_t launch_shoot_overwrite(float* x, const float* frames, const uint8_t* mask, const int32_t* ftab, int64_t N, int32_t O, int64_t rows,
                                  hipStream_t s);
// gathers of blocks of blk floats: dst[e] = src[sb * blk + (gid ? gid[(e mod blk) / width] * width + e mod width : e mod blk)], e < n, with
// sb = idx ? idx[e / blk] : (e / blk) mod src_blocks -- per-window rows out of a trajectory (idx: the frame of every block), a static array
// replicated (src_blocks = 1), a trajectory into the engine's node order (gid)
hipError_t launch_shoot_gather(float* dst, const float* src, int64_t n, int64_t blk, int64_t src_blocks, const int32_t* idx, const int32_t* gid,
                               int32_t width, hipStream_t s);
hipError_t launch_shoot_gather_u8(uint8_t* dst, const uint8_t* src, int64_t n, int64_t blk, hipStream_t s);   // dst[e] = src[e mod blk]
// acc[i] = (first ? 0 : acc[i]) + g[i] in double; out[i] = (float)acc[i]
hipError_t launch_grad_accum(const float* g, double* acc, int64_t n, bool first, hipStream_t s);
hipError_t launch_grad_finish(const double* acc, float* out, int64_t n, hipStream_t s);

}  // namespace mgn
