// C ABI of the engine (include/mgn_hip.h).  Host orchestration only: parameter repacking into MFMA
// fragment order, device buffers, kernel sequencing.  All arithmetic is in kernels.hip; there is no
// CPU compute path here.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <string>
#include <sys/stat.h>
#include <unistd.h>
#include <vector>

#include "engine_internal.h"
#include "train.h"
#include "graph_dev.h"
#include "launch.hpp"

using namespace mgn;


namespace {

thread_local std::string g_create_error;

}  // namespace

namespace mgn {

int fail(mgn_engine* h, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (h) h->err = buf; else g_create_error = buf;
    return code;
}

// The width rule of everything that computes on the training kernels (mgn_train.cpp, train.hip): they pad every input to L columns
// (k_affine_pad), describe an encoder's first layer as one block of at most L rows and index the decoder's output in rows of L, so
// Fn, Fe, Fe2 (with two edge sets) and O are at most L there.  The name of the first width above L (its value in *w), or null.
const char* width_over_L(const mgn_config& c, int* w) {
    const struct { const char* name; int v; } ws[] = {{"Fn", c.Fn}, {"Fe", c.Fe}, {"Fe2", c.n_edge_sets == 2 ? c.Fe2 : 0}, {"O", c.O}};
    for (const auto& x : ws)
        if (x.v > c.L) { *w = x.v; return x.name; }
    return nullptr;
}
// ... as the refusal of a training entry point: before the device check (a host-only handle answers it too), any allocation, launch or
// collective -- every rank of a group holds the same widths, so all of them stop here
int width_refuse(mgn_engine* h, const char* who) {
    int w = 0;
    if (const char* name = width_over_L(h->cfg, &w))
        return fail(h, MGN_E_UNSUPPORTED, "%s: %s = %d exceeds L = %d: the training kernels take Fn, Fe, Fe2, O <= L (inference with ln_dims = MGN_LN_ROWS serves any width)", who, name, w, h->cfg.L);
    return MGN_OK;
}

}  // namespace mgn

namespace {

bool cfg_ok(const mgn_config* c, std::string& why) {
    if (!c) { why = "null config"; return false; }
    if (c->Fn < 1 || c->Fe < 1 || c->O < 1) { why = "Fn, Fe, O must be >= 1"; return false; }
    if (c->L != 32 && c->L != 64 && c->L != 128) { why = "L must be 32, 64 or 128 on the HIP path"; return false; }
    if (c->hidden_layers < 1 || c->hidden_layers > 4) { why = "hidden_layers must be 1 .. 4 on the HIP path"; return false; }
    if (c->mps < 1) { why = "mps must be >= 1"; return false; }
    if (c->dtype != MGN_F32 && c->dtype != MGN_BF16) { why = "dtype must be MGN_F32 or MGN_BF16"; return false; }
    if (c->dtype == MGN_BF16 && (c->L != 128 || c->hidden_layers != 2)) { why = "MGN_BF16 is implemented for L = 128, hidden_layers = 2"; return false; }
    if (c->nranks < 1 || c->rank < 0 || c->rank >= c->nranks) { why = "bad rank/nranks"; return false; }
    if (c->n_edge_sets < 0 || c->n_edge_sets > MAX_EDGE_SETS) { why = "n_edge_sets must be 0, 1 or 2"; return false; }
    if (c->n_edge_sets == 2 && c->Fe2 < 1) { why = "Fe2 must be >= 1 with two edge sets"; return false; }
    if (c->ln_mode != MGN_LN_VAR_EPS && c->ln_mode != MGN_LN_STD_EPS) { why = "ln_mode must be MGN_LN_VAR_EPS or MGN_LN_STD_EPS"; return false; }
    if (c->ln_dims != MGN_LN_ROWS && c->ln_dims != MGN_LN_ALL) { why = "ln_dims must be MGN_LN_ROWS or MGN_LN_ALL"; return false; }
    if (c->ln_dims == MGN_LN_ALL && (c->dtype != MGN_F32 || c->nranks != 1 || c->n_edge_sets > 1)) {
        why = "ln_dims = MGN_LN_ALL (whole-array LayerNorm) runs in fp32 on one partition with one edge set";
        return false;
    }
    if (c->ln_dims == MGN_LN_ALL) {                        // (every compute path of that mode runs on the training kernels: lnall_*)
        int w = 0;
        if (const char* name = mgn::width_over_L(*c, &w)) {
            why = std::string("ln_dims = MGN_LN_ALL computes on the training kernels, which take Fn, Fe, Fe2, O <= L: ") + name + " = " + std::to_string(w) + ", L = " + std::to_string(c->L);
            return false;
        }
    }
    return true;
}

// MGN-spec MLP: Dense(in -> L) . ReLU -> [Dense(L -> L) . ReLU] x (hidden_layers - 1) -> Dense(L -> out) [+ LayerNorm]
size_t mlp_layout(MlpOff& m, size_t off, int in, int L, int out, bool ln, int hidden_layers) {
    int dims[MAX_DENSE + 1];
    const int nl = hidden_layers + 1;
    dims[0] = in;
    for (int i = 1; i < nl; ++i) dims[i] = L;
    dims[nl] = out;
    m.in = in;
    m.out = out;
    m.ln = ln;
    m.nl = nl;
    for (int i = 0; i < nl; ++i) {
        m.W[i] = off;
        off += (size_t)dims[i] * dims[i + 1];
        m.b[i] = off;
        off += dims[i + 1];
    }
    if (ln) {
        m.gamma = off;
        off += out;
        m.beta = off;
        off += out;
    }
    return off;
}

size_t layout_all(mgn_engine* h) {
    const mgn_config& c = h->cfg;
    size_t off = 0;
    off = mlp_layout(h->enc_node, off, c.Fn, c.L, c.L, true, c.hidden_layers);
    // MGN-spec order: encoder-node, encoder-edge per set, (edge MLP per set, node MLP) x mps, decoder
    h->nsets = c.n_edge_sets == 2 ? 2 : 1;
    h->es[0].Fe = c.Fe;
    h->es[1].Fe = c.Fe2;
    for (int q = 0; q < h->nsets; ++q) {
        off = mlp_layout(h->es[q].enc, off, h->es[q].Fe, c.L, c.L, true, c.hidden_layers);
        h->es[q].pe.resize(c.mps);
    }
    h->pn.resize(c.mps);
    for (int k = 0; k < c.mps; ++k) {
        for (int q = 0; q < h->nsets; ++q) off = mlp_layout(h->es[q].pe[k], off, 3 * c.L, c.L, c.L, true, c.hidden_layers);
        off = mlp_layout(h->pn[k], off, (1 + h->nsets) * c.L, c.L, c.L, true, c.hidden_layers);
    }
    off = mlp_layout(h->dec, off, c.L, c.L, c.O, false, c.hidden_layers);
    return off;
}

inline int phi(int j, int hh) { return 32 * (j >> 4) + (j & 3) + 8 * ((j & 15) >> 2) + 4 * hh; }

}  // namespace
namespace mgn {
// L x L chunk of W (row-major [K][ldw], rows kbase.., all L output columns) -> fragment order
void pack_chunk(float* dst, const float* W, int ldw, int kbase, int L) {
    const int NT = L / 32, J = L / 2;
    for (int j = 0; j < J; ++j)
        for (int lane = 0; lane < 64; ++lane) {
            const int hh = lane >> 5, i = lane & 31;
            const float* wrow = W + (size_t)(kbase + phi(j, hh)) * ldw;
            for (int t = 0; t < NT; ++t) dst[((size_t)j * 64 + lane) * NT + t] = wrow[32 * t + i];
        }
}
// t-major copy of a packed chunk, four consecutive k-steps per lane contiguous: [t][j/4][lane][j%4] (cooperative kernels)
void pack_chunk_tmajor(float* dst, const float* frag, int L) {
    const int NT = L / 32, J = L / 2;
    for (int t = 0; t < NT; ++t)
        for (int j = 0; j < J; ++j)
            for (int lane = 0; lane < 64; ++lane)
                dst[(((size_t)t * (J / 4) + j / 4) * 64 + lane) * 4 + (j & 3)] = frag[((size_t)j * 64 + lane) * NT + t];
}
// 128 x 128 chunk of W (row-major [K][ldw], rows kbase..) -> v_mfma_f32_16x16x4_f32 fragment order of the 16-row cooperative
// kernels: wave w owns output blocks 2w, 2w+1 (16 features each); k-step (bb, i) contracts the four input features
// 16 bb + 4 q + i (q = lane >> 4), i.e. register (bb, i) of every lane's row fragment:
//   dst[(((w*8 + bb)*2 + j)*64 + lane)*4 + i] = W[kbase + 16 bb + 4 (lane>>4) + i][16 (2w + j) + (lane & 15)]
void pack_chunk16(float* dst, const float* W, int ldw, int kbase) {
    for (int w = 0; w < 4; ++w)
        for (int bb = 0; bb < 8; ++bb)
            for (int j = 0; j < 2; ++j)
                for (int lane = 0; lane < 64; ++lane)
                    for (int i = 0; i < 4; ++i)
                        dst[((((size_t)w * 8 + bb) * 2 + j) * 64 + lane) * 4 + i] =
                            W[(size_t)(kbase + 16 * bb + 4 * (lane >> 4) + i) * ldw + 16 * (2 * w + j) + (lane & 15)];
}
// vector of L values (stride between consecutive features = stride) -> table fragment order
void pack_tab(float* dst, const float* vec, int L, int stride) {
    for (int m = 0; m < L / 8; ++m)
        for (int hh = 0; hh < 2; ++hh)
            for (int i = 0; i < 4; ++i)
                dst[(m * 2 + hh) * 4 + i] = vec ? vec[(size_t)(32 * (m >> 2) + 8 * (m & 3) + 4 * hh + i) * stride] : 0.f;
}
}  // namespace mgn
namespace {

inline uint16_t f32_to_bf16(float f) {   // round to nearest even (inputs are finite weights / latents)
    uint32_t u;
    memcpy(&u, &f, 4);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
// feature held by element j of piece (s, hh) of a bf16 row fragment (see kernels.hip, bf16 section)
inline int bf_feature(int sidx, int hh, int j) { return 32 * (sidx >> 1) + 16 * (sidx & 1) + 8 * (j >> 2) + 4 * hh + (j & 3); }
inline float bf16_to_f32(uint16_t b) {
    const uint32_t u = (uint32_t)b << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
// the same chunk as three bf16 pieces with w = hi + mid + lo exactly (dst: 3 x 16384, each in the fragment order below)
void pack_chunk_bf16(uint16_t* dst, const float* W, int ldw, int kbase);
void pack_chunk16_bf16(uint16_t* dst, const float* W, int ldw, int kbase);
void pack_chunk_split(uint16_t* dst, const float* W, int ldw, int kbase, bool frag16 = false) {
    std::vector<float> r1((size_t)128 * 128), r2((size_t)128 * 128), w0((size_t)128 * 128);
    for (int k = 0; k < 128; ++k)
        for (int n = 0; n < 128; ++n) {
            const float w = W[(size_t)(kbase + k) * ldw + n];
            const float a = bf16_to_f32(f32_to_bf16(w));
            const float ra = w - a;
            const float b = bf16_to_f32(f32_to_bf16(ra));
            w0[(size_t)k * 128 + n] = w;
            r1[(size_t)k * 128 + n] = ra;
            r2[(size_t)k * 128 + n] = ra - b;
        }
    auto pk = frag16 ? pack_chunk16_bf16 : pack_chunk_bf16;
    pk(dst, w0.data(), 128, 0);
    pk(dst + 16384, r1.data(), 128, 0);
    pk(dst + 2 * 16384, r2.data(), 128, 0);
}
// the same chunk times a power of two as two fp16 pieces, w scale = hi + lo (+ <= 2^-23 relative; split_common.hpp), both round to nearest
// even (dst: 2 x 16384, the bf16 pieces' fragment order)
void pack_chunk_split_h(uint16_t* dst, const float* W, int ldw, int kbase, float scale, bool frag16 = false) {
    auto put = [&](size_t at, int k, int n) {
        const float ws = W[(size_t)(kbase + k) * ldw + n] * scale;
        const _Float16 hi = (_Float16)ws;
        const _Float16 lo = (_Float16)(ws - (float)hi);
        memcpy(&dst[at], &hi, 2);
        memcpy(&dst[16384 + at], &lo, 2);
    };
    if (frag16) {                                        // [ks][ob][lane][8] (pack_chunk16_bf16's order)
        for (int ks = 0; ks < 4; ++ks)
            for (int ob = 0; ob < 8; ++ob)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 8; ++j)
                        put((((size_t)ks * 8 + ob) * 64 + lane) * 8 + j, 16 * (2 * ks + (j >> 2)) + 4 * (lane >> 4) + (j & 3), 16 * ob + (lane & 15));
        return;
    }
    for (int sidx = 0; sidx < 8; ++sidx)
        for (int t = 0; t < 4; ++t)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 8; ++j)
                    put((((size_t)sidx * 4 + t) * 64 + lane) * 8 + j, bf_feature(sidx, lane >> 5, j), 32 * t + (lane & 31));
}
// the A fragments of v_mfma_f32_16x16x32_bf16 (the 16-row kernels of kernels.hip on the split path): step (ks, ob) = output block ob of k-step ks; lane
// (r16 = lane & 15, g = lane >> 4) holds output 16 ob + r16, its element j input 16 (2 ks + (j >> 2)) + 4 g + (j & 3) -- the order in
// which a lane's two accumulator blocks 2 ks, 2 ks + 1 of the layer before hold them
void pack_chunk16_bf16(uint16_t* dst, const float* W, int ldw, int kbase) {
    for (int ks = 0; ks < 4; ++ks)
        for (int ob = 0; ob < 8; ++ob)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 8; ++j) {
                    const int k = 16 * (2 * ks + (j >> 2)) + 4 * (lane >> 4) + (j & 3), n = 16 * ob + (lane & 15);
                    dst[(((size_t)ks * 8 + ob) * 64 + lane) * 8 + j] = f32_to_bf16(W[(size_t)(kbase + k) * ldw + n]);
                }
}
// 128 x 128 chunk of W (row-major [K][ldw], rows kbase..) -> bf16 fragment order [s][t][lane][8]
void pack_chunk_bf16(uint16_t* dst, const float* W, int ldw, int kbase) {
    for (int sidx = 0; sidx < 8; ++sidx)
        for (int t = 0; t < 4; ++t)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 8; ++j) {
                    const int hh = lane >> 5, i = lane & 31;
                    dst[(((size_t)sidx * 4 + t) * 64 + lane) * 8 + j] = f32_to_bf16(W[(size_t)(kbase + bf_feature(sidx, hh, j)) * ldw + 32 * t + i]);
                }
}

}  // namespace
namespace mgn {
int need(mgn_engine* h, bool params, bool graph, bool packed, bool lnall_ok) {
    if (!h) return MGN_E_ARG;
    if (h->host_only) return fail(h, MGN_E_HIP, "host-only handle (MGN_DEVICE_NONE): no compute path; create the handle on a HIP device");
    // whole-array LayerNorm couples every row of an MLP's output: the fused kernels behind the other compute entry points cannot
    // compute it (mgn_forward and mgn_processor_steps branch off to the unfused driver before they get here)
    if (params && graph && h->cfg.ln_dims == MGN_LN_ALL && !lnall_ok)
        return fail(h, MGN_E_UNSUPPORTED, "ln_dims = MGN_LN_ALL (whole-array LayerNorm) is not served by this entry point (the staged mgn_fwd_* / mgn_proc_* calls run the fused kernels only)");
    if (params && !h->have_params) return fail(h, MGN_E_STATE, "mgn_set_params has not been called");
    if (graph && !h->have_graph) return fail(h, MGN_E_STATE, "mgn_set_graph has not been called");
    if (params && packed && !h->packed_ok) return pack_inference_weights(h);
    return MGN_OK;
}
}  // namespace mgn
namespace {

struct ProfScope {
    mgn_engine* h;
    int fam;
    hipEvent_t a = nullptr, b = nullptr;
    static hipEvent_t take(mgn_engine* h) {
        hipEvent_t e = nullptr;
        if (!h->event_pool.empty()) {
            e = h->event_pool.back();
            h->event_pool.pop_back();
        } else if (hipEventCreate(&e) != hipSuccess) {
            e = nullptr;
        }
        return e;
    }
    ProfScope(mgn_engine* h_, int fam_) : h(h_), fam(fam_) {
        if (!h->prof) return;
        a = take(h);
        b = take(h);
        if (a && b) (void)hipEventRecord(a, h->stream);
    }
    ~ProfScope() {
        if (a && b) {
            (void)hipEventRecord(b, h->stream);
            h->recs.push_back({fam, a, b});
        }
    }
};

const float* W(const mgn_engine* h, size_t off) { return h->wfrag.as<float>() + off; }

// the device copies of one chunk (ChunkRef) as the kernels' argument blocks take them; null: that copy is not built
struct ChunkPtrs {
    const float *frag, *frag_t;                 // fragment order, t-major
    const uint16_t *sp32, *sp16, *h32, *h16, *bf;
    float s, rs;                                // the fp16 pieces' power of two and its inverse (1 without fp16 pieces)
};
ChunkPtrs chunk_ptrs(const mgn_engine* h, const ChunkRef& r) {
    auto at = [](const DevBuf& b, size_t off) -> const uint16_t* { return off == ChunkRef::NONE ? nullptr : b.as<uint16_t>() + off; };
    ChunkPtrs c{};
    if (r.frag != ChunkRef::NONE) {
        c.frag = W(h, r.frag);
        c.frag_t = c.frag + (size_t)h->cfg.L * h->cfg.L;
    }
    c.sp32 = at(h->wsp, r.sp32);
    c.sp16 = at(h->wsp, r.sp16);
    c.h32 = at(h->wsp, r.h32);
    c.h16 = at(h->wsp, r.h16);
    c.bf = at(h->wbf, r.bf);
    c.s = r.scale;
    c.rs = 1.f / r.scale;
    return c;
}

inline int64_t tiles_or_one(int32_t nt) { return nt > 0 ? nt : 1; }

// per-set buffers (sized by that set's local edges and by the owned + halo nodes)
int alloc_edge_set(mgn_engine* h, int q) {
    const int L = h->cfg.L;
    const LocalGraph& g = h->g;
    auto& es = h->es[q];
    const int64_t nte = tiles_or_one(es.ntiles_e), ntn = tiles_or_one(h->ntiles_n);
    struct { DevBuf* b; size_t bytes; } bufs[5] = {
        {&es.P, (size_t)(g.n_own + g.n_halo + 1 + 16) * L * 4}, {&es.Q, (size_t)(g.n_own + 1 + 16) * L * 4},    // (+ 16: rows live in blocks of eight)
        {&es.Elat, tile_floats(nte, L) * 4}, {&es.AGG, tile_floats(ntn, L) * 4}, {&es.CARRY, (size_t)(4 * nte + 1 + 16) * L * 4}};
    // (CARRY: two rows per 32-edge tile, or per 16-edge tile with the 16-row cooperative kernels; its last row stays zero)
    // padding rows of the tile-major arrays and the zero row of CARRY (its last row) must read as 0
    for (auto& b : bufs) {
        HIPCHK(h, b.b->ensure(b.bytes));
        HIPCHK(h, hipMemsetAsync(b.b->p, 0, b.bytes, h->stream));
    }
    if (h->cfg.dtype == MGN_BF16) {
        struct { DevBuf* b; size_t bytes; } bb[5] = {
            {&es.bElat, tile_floats(nte, L) * 2}, {&es.bAGG, tile_floats(ntn, L) * 2},
            {&es.bP, (size_t)(g.n_own + g.n_halo + 1 + 16) * L * 2}, {&es.bQ, (size_t)(g.n_own + 1 + 16) * L * 2},
            {&es.bCARRY, (size_t)(4 * nte + 1 + 16) * L * 2}};
        for (auto& b : bb) {
            HIPCHK(h, b.b->ensure(b.bytes));
            HIPCHK(h, hipMemsetAsync(b.b->p, 0, b.bytes, h->stream));
        }
    }
    return MGN_OK;
}

void drop_graph(mgn_engine* h) {
    if (h->rhs_exec) (void)hipGraphExecDestroy(h->rhs_exec);
    h->rhs_exec = nullptr;
    h->rhs_warm = false;
    if (h->fwd_exec) (void)hipGraphExecDestroy(h->fwd_exec);
    h->fwd_exec = nullptr;
    h->fwd_warm = false;
    if (h->graph_exec) (void)hipGraphExecDestroy(h->graph_exec);
    h->graph_exec = nullptr;
    h->graph_nsteps = -1;
    h->graph_warm = -1;
}

// run_graphed's size rule for mgn_forward and the resident right-hand sides: launch-bound (small) passes on a capturable stream
// (the legacy NULL stream -- mgn_set_stream(h, NULL) -- cannot be captured: eager there)
bool small_graphable(const mgn_engine* h) { return h->use_graph && !h->prof && h->stream != nullptr && launch_is_small(h->ntiles_n); }

// the 16-row kernels run this handle's processor steps (kernels.hip: coop16_handle): one choice per handle and graph
int32_t use_c16(const mgn_engine* h) {
    int32_t nte[MAX_EDGE_SETS] = {};
    for (int q = 0; q < h->nsets; ++q) nte[q] = h->es[q].ntiles_e;
    return coop16_handle(h->cfg.L, h->cfg.hidden_layers, h->cfg.dtype == MGN_F32, h->nsets, h->ntiles_n, nte) ? 1 : 0;
}
// bf16 storage runs its own pipelined kernels wherever the 16-row kernels do not take the handle
bool bf16_pipe(const mgn_engine* h) { return h->cfg.dtype == MGN_BF16 && !use_c16(h); }

// GenMlp of an MLP: used when hidden_layers != 2 (or when tests force the GEN kernels, kernel path 4)
GenMlp gen_of(const mgn_engine* h, const GenOff& g, bool has_last) {
    GenMlp m{};
    const int nmid = h->cfg.hidden_layers - 1;
    for (int i = 0; i < nmid + (has_last ? 1 : 0); ++i) m.chunk[i] = W(h, g.ch[i]);
    m.tabs = W(h, g.tabs);
    m.nmid = nmid;
    m.use = (h->cfg.hidden_layers != 2 || get_kernel_path() == 4) ? 1 : 0;
    return m;
}

// the weights of an encoder / decoder stage (StageW, kernels.h) from its chunks, its tables and its GenOff
template <int N>
StageW<N> stage_weights(const mgn_engine* h, const ChunkRef (&refs)[N], size_t tabs, const GenOff& g, bool has_last) {
    StageW<N> w{};
    for (int i = 0; i < N; ++i) {
        const ChunkPtrs c = chunk_ptrs(h, refs[i]);
        w.chunk[i] = c.frag;
        w.splith[i] = c.h32;
        w.h2_rs[i] = c.rs;
    }
    w.tabs = W(h, tabs);
    w.gen = gen_of(h, g, has_last);
    return w;
}

EdgeArgs edge_args(mgn_engine* h, int k, int q = 0) {
    EdgeArgs a{};
    auto& es = h->es[q];
    a.snd = es.d_snd.as<int32_t>();
    a.rcv = es.d_rcv.as<int32_t>();
    a.E = h->g.set[q].e_local;
    a.ntiles = es.ntiles_e;
    a.bf = h->cfg.dtype == MGN_BF16 ? 1 : 0;            // (only the 16-row kernels are launched with fp32 EdgeArgs in bf16 mode)
    a.P = a.bf ? es.bP.as<float>() : es.P.as<float>();
    a.Q = a.bf ? es.bQ.as<float>() : es.Q.as<float>();
    a.Elat = a.bf ? es.bElat.as<float>() : es.Elat.as<float>();
    a.AGG = a.bf ? es.bAGG.as<float>() : es.AGG.as<float>();
    a.CARRY = a.bf ? es.bCARRY.as<float>() : es.CARRY.as<float>();
    const auto& so = h->steps[k];
    for (int i = 0; i < 3; ++i) {
        const ChunkPtrs c = chunk_ptrs(h, so.e[q][i]);
        a.chunk[i] = c.frag;
        a.chunk_t[i] = c.frag_t;
        a.split[i] = c.sp32;
        a.split16[i] = c.sp16;
        a.splith[i] = c.h32;
        a.split16h[i] = c.h16;
        a.h2_s[i] = c.s;
        a.h2_rs[i] = c.rs;
    }
    a.tabs = W(h, so.e_tabs[q]);
    a.gen = gen_of(h, so.e_gen[q], true);
    a.h2_b2pos = so.e_b2pos[q];
    a.c16 = use_c16(h);
    if (k == 0 && q == 0 && h->elat_src_override && a.c16 && !a.gen.use) a.ElatSrc = h->elat_src_override;
    constexpr int32_t STAGGER_EDGE = 0;   // start stagger of waves 4..7: none since the padded MFMAs (sweep 0..64: 4.558 .. 4.621 ms)
    a.stagger = STAGGER_EDGE;
    a.tile0 = 0;
    a.stamps = h->d_stamps.as<unsigned long long>();
    return a;
}

// tiles [0, tb) of set q hold every edge with a halo sender (they need the exchanged P rows); tiles [tb, ntiles) do not
inline int32_t boundary_tiles(const mgn_engine* h, int q) {
    const int64_t tb = (h->g.set[q].halo_span + TILE - 1) / TILE;
    return (int32_t)(tb < h->es[q].ntiles_e ? tb : h->es[q].ntiles_e);
}

// the chunk of StepChunks::n that slot i of a node-side argument block takes when the block projects onto set q: the projection of
// set 1 is launched on its own (mode 2) and takes its WP / WQ (7, 8) in the projection slots 4, 5
inline int node_slot(int i, int q) { return q == 1 && (i == 4 || i == 5) ? i + 3 : i; }

// q: the edge set whose P,Q the projection part (modes 1, 2) writes
NodeArgs node_args(mgn_engine* h, int k, int mode, int q = 0) {
    NodeArgs a{};
    const auto& so = h->steps[k];
    a.n = h->g.n_own;
    a.ntiles = h->ntiles_n;
    a.rowptr = h->es[0].d_rowptr.as<int32_t>();
    const bool bf = h->cfg.dtype == MGN_BF16;           // (only the 16-row kernels are launched with fp32 NodeArgs in bf16 mode)
    a.bf = bf ? 1 : 0;
    a.V = bf ? h->bV.as<float>() : h->V.as<float>();
    a.AGG = bf ? h->es[0].bAGG.as<float>() : h->es[0].AGG.as<float>();
    a.CARRY = bf ? h->es[0].bCARRY.as<float>() : h->es[0].CARRY.as<float>();
    a.P = bf ? h->es[q].bP.as<float>() : h->es[q].P.as<float>();
    a.Q = bf ? h->es[q].bQ.as<float>() : h->es[q].Q.as<float>();
    a.tabs = W(h, q == 1 ? so.p1_tabs : so.n_tabs);
    const bool agg2 = h->nsets > 1 && mode != 2;        // the node MLP reads the second set's aggregate
    if (agg2) {
        a.rowptr2 = h->es[1].d_rowptr.as<int32_t>();
        a.AGG2 = bf ? h->es[1].bAGG.as<float>() : h->es[1].AGG.as<float>();
        a.CARRY2 = bf ? h->es[1].bCARRY.as<float>() : h->es[1].CARRY.as<float>();
        a.zero_row2 = 4 * tiles_or_one(h->es[1].ntiles_e);
        if (q == 0) {                                   // the 16-row kernels project both sets in one launch (mode 1)
            a.P2 = bf ? h->es[1].bP.as<float>() : h->es[1].P.as<float>();
            a.Q2 = bf ? h->es[1].bQ.as<float>() : h->es[1].Q.as<float>();
            a.tabs2 = W(h, so.p1_tabs);
        }
    }
    // A copy that is not built binds as null (slots 6 .. 8 with one edge set; the 32x32x16 pieces in bf16 storage).  The other
    // conditions are policy -- what the kernels are given:
    const bool projects_both = agg2 && q == 0;          // fp32 chunks 7, 8 (6: to every launch that runs the node MLP of two sets)
    const bool set1_projection = q == 1;                // gets none of the node MLP's three-bf16-piece chunks 0 .. 3 in the 32x32x16 order
    const bool fp16_pieces32 = h->nsets == 1;           // two fp16 pieces, 32x32x16 order: k_node_split_h / k_project_split_h, one edge set only
    for (int i = 0; i < 9; ++i) {
        const ChunkPtrs c = chunk_ptrs(h, so.n[node_slot(i, q)]);
        if (i < 6 || (i == 6 && agg2) || (i > 6 && projects_both)) {
            a.chunk[i] = c.frag;
            a.chunk_t[i] = c.frag_t;
        }
        if (i < 7 && !(set1_projection && i < 4)) a.split[i] = c.sp32;
        if (i < 6 && fp16_pieces32) a.splith[i] = c.h32;
        a.split16[i] = c.sp16;
        a.split16h[i] = c.h16;
        a.h2_s[i] = c.s;
        a.h2_rs[i] = c.rs;
    }
    a.h2_b2pos = a.splith[0] ? so.n_b2pos : 0.f;
    a.mode = mode;
    a.gen = gen_of(h, so.n_gen, true);
    constexpr int32_t STAGGER_NODE = 8;   // start stagger of waves 4..7, s_sleep(127) units
    a.stagger = STAGGER_NODE;
    a.zero_row = 4 * tiles_or_one(h->es[0].ntiles_e);
    a.c16 = use_c16(h);
    a.stamps = h->d_stamps.as<unsigned long long>();
    a.tile0 = 0;
    return a;
}

BfEdgeArgs bf_edge_args(mgn_engine* h, int k, int q = 0) {
    BfEdgeArgs a{};
    auto& es = h->es[q];
    a.snd = es.d_snd.as<int32_t>();
    a.rcv = es.d_rcv.as<int32_t>();
    a.E = h->g.set[q].e_local;
    a.ntiles = es.ntiles_e;
    a.P = es.bP.as<uint16_t>();
    a.Q = es.bQ.as<uint16_t>();
    a.Elat = es.bElat.as<uint16_t>();
    a.AGG = es.bAGG.as<uint16_t>();
    a.CARRY = es.bCARRY.as<uint16_t>();
    for (int i = 0; i < 3; ++i) a.chunk[i] = chunk_ptrs(h, h->steps[k].e[q][i]).bf;
    a.tabs = W(h, h->steps[k].e_tabs[q]);
    a.stamps = h->d_stamps.as<unsigned long long>();
    return a;
}

// project: the args feed k_project_bf16_pipe (P,Q of set q); else k_node_bf16_pipe (node MLP over all sets' aggregates)
BfNodeArgs bf_node_args(mgn_engine* h, int k, int q = 0, bool project = false) {
    BfNodeArgs a{};
    const auto& so = h->steps[k];
    a.n = h->g.n_own;
    a.ntiles = h->ntiles_n;
    a.rowptr = h->es[0].d_rowptr.as<int32_t>();
    a.V = h->bV.as<uint16_t>();
    a.AGG = h->es[0].bAGG.as<uint16_t>();
    a.CARRY = h->es[0].bCARRY.as<uint16_t>();
    a.P = h->es[q].bP.as<uint16_t>();
    a.Q = h->es[q].bQ.as<uint16_t>();
    const bool agg2 = h->nsets > 1 && !project;
    for (int i = 0; i < (agg2 ? 7 : 6); ++i) a.chunk[i] = chunk_ptrs(h, so.n[node_slot(i, q)]).bf;
    a.tabs = W(h, q == 1 ? so.p1_tabs : so.n_tabs);
    if (agg2) {
        a.rowptr2 = h->es[1].d_rowptr.as<int32_t>();
        a.AGG2 = h->es[1].bAGG.as<uint16_t>();
        a.CARRY2 = h->es[1].bCARRY.as<uint16_t>();
        a.zero_row2 = 4 * tiles_or_one(h->es[1].ntiles_e);
    }
    a.zero_row = 4 * tiles_or_one(h->es[0].ntiles_e);
    a.tile0 = 0;
    return a;
}

}  // namespace

// ---- shared with the solve drivers (mgn_solve.cpp; declared in engine_internal.h) ----
int mgn::alloc_latents(mgn_engine* h) {
    const int L = h->cfg.L;
    const LocalGraph& g = h->g;
    const int64_t ntn = tiles_or_one(h->ntiles_n);
    HIPCHK(h, h->V.ensure(tile_floats(ntn, L) * 4));
    HIPCHK(h, h->d_out.ensure((size_t)(g.n_own + 1) * h->cfg.O * 4));
    HIPCHK(h, h->d_sum.ensure(4 * sizeof(double)));
    HIPCHK(h, hipMemsetAsync(h->V.p, 0, tile_floats(ntn, L) * 4, h->stream));
    if (h->cfg.dtype == MGN_BF16) {
        HIPCHK(h, h->bV.ensure(tile_floats(ntn, L) * 2));
        HIPCHK(h, hipMemsetAsync(h->bV.p, 0, tile_floats(ntn, L) * 2, h->stream));
    }
    for (int q = 0; q < h->nsets; ++q)
        if (int rc = alloc_edge_set(h, q)) return rc;
    return MGN_OK;
}

// the resident right-hand side (mgn_set_static) and the hipGraph captured over its buffers go together
void mgn::invalidate_static(mgn_engine* h) {
    h->have_static = false;
    h->lnall_edges = false;
    if (h->rhs_exec) {
        if (!h->host_only) (void)hipStreamSynchronize(h->stream);
        (void)hipGraphExecDestroy(h->rhs_exec);
    }
    h->rhs_exec = nullptr;
    h->rhs_warm = false;
}

int mgn::sync_norms_host(mgn_engine* h) {
    if (!h->norms_host_stale) return MGN_OK;
    const size_t n = (size_t)2 * (h->cfg.Fn + h->cfg.Fe + h->cfg.O);
    h->norms_host.resize(n);
    HIPCHK(h, hipMemcpyAsync(h->norms_host.data(), h->norms.p, n * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->norms_host_stale = false;
    return MGN_OK;
}

// step 0's edge launch can read its e rows from a second array (EdgeArgs::ElatSrc): one edge set on the 16-row kernels, one partition
// (in place of a restore copy per right-hand side)
bool mgn::elat_src_ok(mgn_engine* h) { return h->nsets == 1 && h->cfg.nranks == 1 && use_c16(h); }

bool mgn::is_bf16(const mgn_engine* h) { return h->cfg.dtype == MGN_BF16; }
// tile-major storage: rows padded to whole 32-row tiles
size_t mgn::tile_floats(int64_t ntiles, int L) { return (size_t)ntiles * TILE * L; }

// =================================================================================================
extern "C" {

int mgn_abi_version(void) { return MGN_ABI_VERSION; }

int mgn_create(const mgn_config* cfg, mgn_handle** out) try {
    if (!out) return fail(nullptr, MGN_E_ARG, "null out pointer");
    *out = nullptr;
    // P / Q / CARRY rows are addressed through frag.hpp: prow_ptr in two translation units; objects compiled with different
    // MGN_PROW_BLOCK link without complaint and gather garbage
    if (kernels_prow_block() != split_prow_block())
        return fail(nullptr, MGN_E_STATE, "mgn_create: this library was linked from objects that disagree on the P / Q row layout (MGN_PROW_BLOCK %d in kernels.hip, %d in split.hip): rebuild all of it",
                    kernels_prow_block(), split_prow_block());
    std::string why;
    if (!cfg_ok(cfg, why)) return fail(nullptr, MGN_E_ARG, "mgn_create: %s", why.c_str());
    if (cfg->device == MGN_DEVICE_NONE) {
        mgn_engine* ho = new (std::nothrow) mgn_engine();
        if (!ho) return fail(nullptr, MGN_E_OOM, "host allocation failed");
        ho->cfg = *cfg;
        ho->host_only = true;
        layout_all(ho);
        *out = ho;
        return MGN_OK;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, MGN_E_HIP, "mgn_create: no HIP device available (this engine has no CPU fallback)");
    if (cfg->device >= 0) {
        if (cfg->device >= ndev) return fail(nullptr, MGN_E_ARG, "mgn_create: device %d out of range (%d devices)", cfg->device, ndev);
        if (hipSetDevice(cfg->device) != hipSuccess) return fail(nullptr, MGN_E_HIP, "mgn_create: hipSetDevice failed");
    }
    mgn_engine* h = new (std::nothrow) mgn_engine();
    if (!h) return fail(nullptr, MGN_E_OOM, "host allocation failed");
    h->cfg = *cfg;
    if (hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking) != hipSuccess) {
        delete h;
        return fail(nullptr, MGN_E_HIP, "mgn_create: hipStreamCreate failed");
    }
    h->stream = h->own_stream;
    h->use_graph = env_int("MGN_GRAPH", h->use_graph);
    layout_all(h);
    *out = h;
    return MGN_OK;
} MGN_CATCH(nullptr)

void mgn_destroy(mgn_handle* h) {
    if (!h) return;
    if (h->host_only) { delete h->comm; delete h; return; }
    (void)hipStreamSynchronize(h->stream);
    shoot_release(h);
    drop_graph(h);
    for (auto& r : h->recs) {
        (void)hipEventDestroy(r.a);
        (void)hipEventDestroy(r.b);
    }
    for (hipEvent_t e : h->event_pool) (void)hipEventDestroy(e);
    delete h->comm;
    h->comm = nullptr;
    train_free(h);
    if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
    delete h;
}

const char* mgn_last_error(const mgn_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int mgn_set_stream(mgn_handle* h, void* hip_stream) try {
    if (int rc = need(h, false, false)) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    drop_graph(h);
    h->stream = (hip_stream == MGN_STREAM_OWN) ? h->own_stream : reinterpret_cast<hipStream_t>(hip_stream);
    return MGN_OK;
} MGN_CATCH(h)

int mgn_synchronize(mgn_handle* h) try {
    if (int rc = need(h, false, false)) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return MGN_OK;
} MGN_CATCH(h)

size_t mgn_param_count(const mgn_config* c) try {
    std::string why;
    if (!c || c->Fn < 1 || c->Fe < 1 || c->O < 1 || c->L < 1 || c->hidden_layers < 1 || c->hidden_layers > 4 || c->mps < 1) return 0;
    mgn_engine tmp;
    tmp.cfg = *c;
    return layout_all(&tmp);
} MGN_CATCH_SIZE

int mgn_set_params(mgn_handle* h, const float* packed, size_t n) try {
    if (!h || !packed) return fail(h, MGN_E_ARG, "mgn_set_params: null argument");
    if (int rc = need(h, false, false)) return rc;
    const size_t want = layout_all(h);
    if (n != want) return fail(h, MGN_E_ARG, "mgn_set_params: got %zu floats, model needs %zu", n, want);
    // the same values again (a caller that cannot tell whether its parameters changed calls this before every forward: 0.3 ms for the
    // comparison of 9 MB): nothing is invalidated, captured graphs and packed layouts stay
    // (only while the host copy is the authoritative one: after a device-side change it holds older values)
    if (h->have_params && !h->params_host_stale && h->params.size() == n && memcmp(h->params.data(), packed, n * sizeof(float)) == 0) return MGN_OK;
    h->params.assign(packed, packed + n);
    h->params_host_stale = false;
    h->params_dev_ok = false;
    ++h->params_gen;
    train_invalidate(h, 1);
    // The kernels' own weight layouts (three fp32 fragment orders, the bf16 pieces of the split path in two, the bf16 copies) take
    // ~30 ms of host time for the 15-step model; a training loop sets new parameters before EVERY step! and its kernels pack their own
    // (mgn_train.cpp) -- so they are built by the first call that reads them (need()), not here.
    HIPCHK(h, hipStreamSynchronize(h->stream));
    drop_graph(h);
    invalidate_static(h);
    h->packed_ok = false;
    h->have_params = true;
    return MGN_OK;
} MGN_CATCH(h)
}  // extern "C"

namespace mgn {
bool is_device_pointer(const void* p) {
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {   // (memory HIP never saw: an error on some runtimes, "unregistered" on others)
        (void)hipGetLastError();
        return false;
    }
    return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
}

int host_params(mgn_engine* h, const float** p) {
    if (h->params_host_stale) {
        HIPCHK(h, hipMemcpyAsync(h->params.data(), h->d_params.p, h->params.size() * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        h->params_host_stale = false;
    }
    *p = h->params.data();
    return MGN_OK;
}

int dev_params(mgn_engine* h, const float** p) {
    if (!h->params_dev_ok) {
        HIPCHK(h, h->d_params.ensure(h->params.size() * 4));
        HIPCHK(h, hipMemcpyAsync(h->d_params.p, h->params.data(), h->params.size() * 4, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));       // (the host vector may be assigned to again as soon as this returns)
        h->params_dev_ok = true;
    }
    *p = h->d_params.as<float>();
    return MGN_OK;
}

int params_changed_on_device(mgn_engine* h) {
    h->params_dev_ok = true;
    h->params_host_stale = true;
    h->have_params = true;
    h->packed_ok = false;
    ++h->params_gen;
    train_invalidate(h, 1);
    // a captured inference graph must have run before it is destroyed; a training loop holds none and is not waited for
    if (h->graph_exec || h->fwd_exec || h->rhs_exec) HIPCHK(h, hipStreamSynchronize(h->stream));
    drop_graph(h);
    invalidate_static(h);
    return MGN_OK;
}

int set_params_resident(mgn_engine* h, const float* src, size_t n, const char* who) {
    const size_t want = layout_all(h);
    if (n != want) return fail(h, MGN_E_ARG, "%s: got %zu floats, model needs %zu", who, n, want);
    const bool from_device = is_device_pointer(src);
    HIPCHK(h, h->d_params.ensure(n * 4));
    HIPCHK(h, hipMemcpyAsync(h->d_params.p, src, n * 4, hipMemcpyDefault, h->stream));
    if (!from_device) HIPCHK(h, hipStreamSynchronize(h->stream));   // (pageable memory: it has left the caller's array on return)
    if (h->params.size() != n) h->params.resize(n);                  // (its length is the model's size everywhere; its values are stale)
    return params_changed_on_device(h);
}
}  // namespace mgn

extern "C" {
int mgn_set_params_dev(mgn_handle* h, const float* packed, size_t n) try {
    if (!h || !packed) return fail(h, MGN_E_ARG, "mgn_set_params_dev: null argument");
    if (n != layout_all(h)) return fail(h, MGN_E_ARG, "mgn_set_params_dev: got %zu floats, model needs %zu", n, layout_all(h));
    if (int rc = need(h, false, false)) return rc;
    return set_params_resident(h, packed, n, "mgn_set_params_dev");
} MGN_CATCH(h)

int mgn_get_params_dev(mgn_handle* h, float* packed, size_t n) try {
    if (!h || !packed) return fail(h, MGN_E_ARG, "mgn_get_params_dev: null argument");
    if (n != layout_all(h)) return fail(h, MGN_E_ARG, "mgn_get_params_dev: got %zu floats, model needs %zu", n, layout_all(h));
    if (int rc = need(h, true, false, false)) return rc;
    const float* dp = nullptr;
    if (int rc = dev_params(h, &dp)) return rc;
    HIPCHK(h, hipMemcpyAsync(packed, dp, n * 4, hipMemcpyDefault, h->stream));
    if (!is_device_pointer(packed)) HIPCHK(h, hipStreamSynchronize(h->stream));
    return MGN_OK;
} MGN_CATCH(h)

int mgn_adam_init(mgn_handle* h, const mgn_adam_desc* a) try {
    if (!h || !a) return fail(h, MGN_E_ARG, "mgn_adam_init: null argument");
    if (!(std::isfinite(a->eta) && std::isfinite(a->beta1) && std::isfinite(a->beta2) && std::isfinite(a->epsilon)) ||
        !(a->eta > 0.f) || !(a->beta1 >= 0.f && a->beta1 < 1.f) || !(a->beta2 >= 0.f && a->beta2 < 1.f) || !(a->epsilon > 0.f))
        return fail(h, MGN_E_ARG, "mgn_adam_init: Adam needs finite eta > 0, 0 <= beta1, beta2 < 1 and epsilon > 0 (got %g, (%g, %g), %g)",
                    (double)a->eta, (double)a->beta1, (double)a->beta2, (double)a->epsilon);
    if (int rc = need(h, false, false)) return rc;
    const size_t bytes = layout_all(h) * 4;
    HIPCHK(h, h->adam_m.ensure(bytes));
    HIPCHK(h, h->adam_v.ensure(bytes));
    HIPCHK(h, hipMemsetAsync(h->adam_m.p, 0, bytes, h->stream));
    HIPCHK(h, hipMemsetAsync(h->adam_v.p, 0, bytes, h->stream));
    h->adam = *a;
    h->adam_beta_t[0] = (double)a->beta1;
    h->adam_beta_t[1] = (double)a->beta2;
    h->adam_ready = true;
    return MGN_OK;
} MGN_CATCH(h)

int mgn_adam_update(mgn_handle* h, const float* grads, size_t n_grads) try {
    if (!h || !grads) return fail(h, MGN_E_ARG, "mgn_adam_update: null argument");
    if (n_grads != layout_all(h)) return fail(h, MGN_E_ARG, "mgn_adam_update: grads has %zu floats, model has %zu", n_grads, layout_all(h));
    if (int rc = need(h, false, false)) return rc;
    if (!h->adam_ready) return fail(h, MGN_E_STATE, "mgn_adam_update: mgn_adam_init has not been called");
    if (!h->have_params) return fail(h, MGN_E_STATE, "mgn_adam_update: no parameters have been set (mgn_set_params / mgn_set_params_dev)");
    const float* dp = nullptr;
    if (int rc = dev_params(h, &dp)) return rc;
    const float* g = grads;
    if (!is_device_pointer(grads)) {
        HIPCHK(h, h->adam_g.ensure(n_grads * 4));
        HIPCHK(h, hipMemcpyAsync(h->adam_g.p, grads, n_grads * 4, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));       // (pageable memory: it has left the caller's array on return)
        g = h->adam_g.as<float>();
    } else if (reinterpret_cast<uintptr_t>(grads) & 15) {   // (the kernel's 16-byte accesses: a view into a larger device array goes through the staging buffer)
        HIPCHK(h, h->adam_g.ensure(n_grads * 4));
        HIPCHK(h, hipMemcpyAsync(h->adam_g.p, grads, n_grads * 4, hipMemcpyDeviceToDevice, h->stream));
        g = h->adam_g.as<float>();
    }
    const mgn_adam_desc& a = h->adam;
    const float c1 = (float)(1.0 - h->adam_beta_t[0]), c2 = (float)(1.0 - h->adam_beta_t[1]);
    HIPCHK(h, launch_adam(h->d_params.as<float>(), h->adam_m.as<float>(), h->adam_v.as<float>(), g, (int64_t)n_grads, a.eta, a.beta1, a.beta2,
                          a.epsilon, c1, c2, h->stream));
    h->adam_beta_t[0] *= (double)a.beta1;
    h->adam_beta_t[1] *= (double)a.beta2;
    return params_changed_on_device(h);
} MGN_CATCH(h)

int mgn_adam_state(mgn_handle* h, int32_t write, float* mt, float* vt, double beta_t[2]) try {
    if (!h || !mt || !vt || !beta_t) return fail(h, MGN_E_ARG, "mgn_adam_state: null argument");
    if (write != 0 && write != 1) return fail(h, MGN_E_ARG, "mgn_adam_state: write must be 0 or 1, got %d", write);
    if (write && !(std::isfinite(beta_t[0]) && std::isfinite(beta_t[1])))
        return fail(h, MGN_E_ARG, "mgn_adam_state: beta_t is not finite");
    if (int rc = need(h, false, false)) return rc;
    if (!h->adam_ready) return fail(h, MGN_E_STATE, "mgn_adam_state: mgn_adam_init has not been called");
    const size_t bytes = layout_all(h) * 4;
    if (write) {
        HIPCHK(h, hipMemcpyAsync(h->adam_m.p, mt, bytes, hipMemcpyDefault, h->stream));
        HIPCHK(h, hipMemcpyAsync(h->adam_v.p, vt, bytes, hipMemcpyDefault, h->stream));
        h->adam_beta_t[0] = beta_t[0];
        h->adam_beta_t[1] = beta_t[1];
    } else {
        HIPCHK(h, hipMemcpyAsync(mt, h->adam_m.p, bytes, hipMemcpyDefault, h->stream));
        HIPCHK(h, hipMemcpyAsync(vt, h->adam_v.p, bytes, hipMemcpyDefault, h->stream));
        beta_t[0] = h->adam_beta_t[0];
        beta_t[1] = h->adam_beta_t[1];
    }
    if (!is_device_pointer(mt) || !is_device_pointer(vt)) HIPCHK(h, hipStreamSynchronize(h->stream));
    return MGN_OK;
} MGN_CATCH(h)
}  // extern "C"

namespace mgn {
// the power of two that puts the largest entry of an L x L chunk (L rows of L floats at W) into [2^14, 2^15): its two fp16 pieces
// are taken of the chunk times it (split_common.hpp)
static float fp16_chunk_scale(const float* W, int L) {
    float mx = 0.f;
    for (size_t i = 0; i < (size_t)L * L; ++i) mx = std::max(mx, std::fabs(W[i]));
    int e = 0;
    (void)std::frexp(mx, &e);                                   // mx = m 2^e, m in [0.5, 1): floor(log2 mx) = e - 1
    if (!(mx > 0.f) || e - 1 < -40) e = -39;
    if (!std::isfinite(mx)) e = 128;
    return std::ldexp(1.f, 15 - e);
}

int pack_inference_weights(mgn_engine* h) {
    layout_all(h);
    const float* p = nullptr;                         // (the small tables and the fp16 scales are formed on the host: its copy, refreshed)
    if (int rc = host_params(h, &p)) return rc;
    const mgn_config& c = h->cfg;
    const int L = c.L;
    const size_t CH = (size_t)L * L, TB = (size_t)T_COUNT * L;

    // The L x L chunks -- all but a megabyte of the ~60 MB of layouts -- are written ON THE DEVICE from the uploaded parameter vector
    // (train.hip: k_pack_weights; the host twins pack_chunk / pack_chunk_tmajor / pack_chunk16 / pack_chunk_bf16 / pack_chunk16_bf16
    // stay as their specification): the host describes them (WPackJob) and keeps packing the small things (tables, first-layer
    // vectors) into `f`, whose chunk regions stay empty and are not uploaded (segments between them are).  30 ms -> ~3 ms per
    // parameter change.
    std::vector<float> f;
    std::vector<WPackJob> jobs;
    std::vector<std::pair<size_t, size_t>> small;           // [begin, end) of what the host packed itself
    size_t seg0 = 0;
    // every chunk is stored three times: [lane-interleaved fragment order][t-major order (cooperative 32-row kernels)]
    // [16x16x4 fragment order (cooperative 16-row kernels, L = 128)]: copies of the chunk at offset `off` live at off + CH, off + 2 CH
    auto add_chunk = [&](const float* Wm, int kbase) {
        const size_t off = f.size();
        if (off > seg0) small.push_back({seg0, off});
        f.resize(off + 3 * CH);
        seg0 = off + 3 * CH;
        jobs.push_back({0, (long long)off, (long long)(Wm - p), L, kbase, 1.f});
        return off;
    };
    // Which copies a chunk gets, by its role (ChunkRef, engine_internal.h) -- the one place that decides it.  The 16-bit pieces exist
    // where the tuned kernels that take them do: L = 128, hidden_layers = 2; in the 16x16x32 order for the 16-row kernels of small
    // meshes (in bf16 storage too, where they keep fp32-accurate arithmetic), in the 32x32x16 order for the 32-row kernels of split.hip
    // (fp32 storage only), which are also the encoders' and the decoder's.
    enum : unsigned { FRAG = 1, SP32 = 2, SP16 = 4, H32 = 8, H16 = 16, BF = 32 };
    const bool pieces = L == 128 && c.hidden_layers == 2, f32 = c.dtype == MGN_F32;
    const unsigned PROC = FRAG | (f32 ? 0 : BF) | (pieces ? SP16 | H16 : 0) | (pieces && f32 ? SP32 | H32 : 0);
    // node-side chunks 6 .. 8 of the second edge set: NodeArgs::splith has no slot for them.  (With two edge sets node_args binds no
    // splith at all, so the h32 copies of chunks 0 .. 5 are as unread there; they are built as they always were.)
    const unsigned PROC_SET1 = PROC & ~H32;
    const unsigned ENDS = FRAG | (pieces && f32 ? H32 : 0);  // encoders, decoder
    // builds the copies in `want` that r does not hold yet, of rows [kbase, kbase + L) of the L-column matrix Wm
    size_t sp_size = 0, bf_size = 0;                         // elements of wsp, wbf
    auto place = [&](ChunkRef& r, const float* Wm, int kbase, unsigned want) {
        if ((want & FRAG) && r.frag == ChunkRef::NONE) r.frag = add_chunk(Wm, kbase);
        if ((want & (H32 | H16)) && r.h32 == ChunkRef::NONE && r.h16 == ChunkRef::NONE) r.scale = fp16_chunk_scale(Wm + (size_t)kbase * L, L);
        auto copy = [&](unsigned bit, size_t& at, int kind, size_t& end, size_t n) {
            if (!(want & bit) || at != ChunkRef::NONE) return;
            jobs.push_back({kind, (long long)end, (long long)(Wm - p), L, kbase, kind >= 4 ? r.scale : 1.f});
            at = end;
            end += n;
        };
        copy(SP32, r.sp32, 1, sp_size, 3 * CH);              // (16-bit copies exist at L = 128 only: CH = 16384, the piece size of WPackJob)
        copy(SP16, r.sp16, 2, sp_size, 3 * CH);
        copy(H32, r.h32, 4, sp_size, 2 * CH);
        copy(H16, r.h16, 5, sp_size, 2 * CH);
        copy(BF, r.bf, 3, bf_size, CH);
    };
    auto add_tabs = [&](const float* b1, const float* b2, const float* b3, const float* ga, const float* be, const float* bq) {
        const size_t off = f.size();
        f.resize(off + 2 * TB);          // fragment order, then natural feature order (16-row kernels)
        const float* src[T_COUNT] = {b1, b2, b3, ga, be, bq, nullptr};
        for (int t = 0; t < T_COUNT; ++t) {
            pack_tab(f.data() + off + (size_t)t * L, src[t], L);
            for (int i = 0; i < L; ++i) f[off + TB + (size_t)t * L + i] = src[t] ? src[t][i] : 0.f;
        }
        for (int blk = 0; blk < 2; ++blk) {                    // T_LN: (eps_in, eps_out) of the LayerNorm variant (frag.hpp: ln_rstd)
            f[off + blk * TB + (size_t)T_LN * L + 0] = c.ln_mode == MGN_LN_STD_EPS ? 0.f : 1e-5f;
            f[off + blk * TB + (size_t)T_LN * L + 1] = c.ln_mode == MGN_LN_STD_EPS ? 1e-5f : 0.f;
        }
        return off;
    };
    auto add_w1f = [&](const float* W1, int K) {  // [K][L] -> per-k fragment tables
        const size_t off = f.size();
        f.resize(off + (size_t)K * L);
        for (int k = 0; k < K; ++k) pack_tab(f.data() + off + (size_t)k * L, W1 + (size_t)k * L, L);
        return off;
    };

    const int S = h->nsets;
    const MlpOff& e0 = h->es[0].pe[0];
    const int nl = c.hidden_layers + 1, nmid = nl - 2;      // Dense layers per MLP; L x L middle layers
    const bool h2 = c.hidden_layers == 2;                   // the tuned kernel families are specialised for this
    // the Dense layers after the first one of MLP m (GenOff): middle layers W[1 .. nmid], then the last one when it is L x L
    // (has_last: every MLP but the decoder), and their biases as tables.  Returns through g.
    auto add_gen = [&](const MlpOff& m, bool has_last, GenOff& g) {
        for (int i = 0; i < nmid; ++i) g.ch[i] = add_chunk(p + m.W[1 + i], 0);
        if (has_last) g.ch[nmid] = add_chunk(p + m.W[nl - 1], 0);
        g.tabs = f.size();
        f.resize(f.size() + (size_t)(nmid + 1) * L);
        for (int i = 0; i < nmid; ++i) pack_tab(f.data() + g.tabs + (size_t)i * L, p + m.b[1 + i], L);
        pack_tab(f.data() + g.tabs + (size_t)nmid * L, has_last ? p + m.b[nl - 1] : nullptr, L);
    };
    // the tuned kernels' "W2" / "W3" of MLP m -- its first and its last L x L layer, whose fp32 copies are ch[0] / ch[nmid] of its
    // GEN list g (one and the same chunk at hidden_layers = 1) -- with the copies `want`
    auto place_w23 = [&](ChunkRef& w2, ChunkRef& w3, const MlpOff& m, const GenOff& g, unsigned want) {
        w2.frag = g.ch[0];
        w3.frag = g.ch[nmid];
        place(w2, p + m.W[1], 0, want);
        place(w3, p + m.W[nl - 1], 0, want);
    };
    auto b2 = [&](const MlpOff& m) { return h2 ? p + m.b[1] : nullptr; };
    auto b3 = [&](const MlpOff& m) { return h2 ? p + m.b[2] : nullptr; };
    auto b2pos = [&](const MlpOff& m) {                      // max(0, max b2): with the fp16 pieces' scales, bounds the input of layer 3
        float bp = 0.f;
        for (int i = 0; i < L; ++i) bp = std::max(bp, p[m.b[1] + i]);
        return bp;
    };
    // The walk: every chunk the tuned kernels take is named here, once, with its role.  (The order is that of wfrag: `small` follows it.)
    // encoder, node side (+ projection onto step-0 edge-MLP layer 1 of set 0)
    for (ChunkRef& r : h->en) r = {};
    for (ChunkRef& r : h->de) r = {};
    {
        const MlpOff& m = h->enc_node;
        add_gen(m, true, h->en_gen);
        place_w23(h->en[0], h->en[1], m, h->en_gen, ENDS);
        place(h->en[2], p + e0.W[0], 0, ENDS);
        place(h->en[3], p + e0.W[0], L, ENDS);
        h->en_tabs = add_tabs(p + m.b[0], b2(m), b3(m), p + m.gamma, p + m.beta, p + e0.b[0]);
        h->en_w1f = add_w1f(p + m.W[0], c.Fn);
    }
    for (int q = 0; q < S; ++q) {
        auto& es = h->es[q];
        const MlpOff& m = es.enc;
        es.ee[0] = es.ee[1] = {};
        add_gen(m, true, es.ee_gen);
        place_w23(es.ee[0], es.ee[1], m, es.ee_gen, ENDS);
        es.ee_tabs = add_tabs(p + m.b[0], b2(m), b3(m), p + m.gamma, p + m.beta, nullptr);
        es.ee_w1f = add_w1f(p + m.W[0], es.Fe);
    }
    // node side of step k: the node MLP and the projections onto the next step's edge MLPs (after the last step, and for k = mps --
    // the pseudo-step -- onto step 0's).  Builds the copies so.n[] does not hold yet.
    auto node_side = [&](mgn_engine::StepChunks& so, int k) {
        const bool pseudo = k == c.mps;
        const MlpOff& mn = h->pn[pseudo ? 0 : k];
        const int kn = k + 1 < c.mps ? k + 1 : 0;
        const MlpOff& nx = h->es[0].pe[kn];
        if (!pseudo) add_gen(mn, true, so.n_gen);
        place_w23(so.n[0], so.n[1], mn, so.n_gen, PROC);
        place(so.n[2], p + mn.W[0], 0, PROC);
        place(so.n[3], p + mn.W[0], L, PROC);
        place(so.n[4], p + nx.W[0], 0, PROC);
        place(so.n[5], p + nx.W[0], L, PROC);
        so.n_tabs = pseudo ? add_tabs(nullptr, nullptr, nullptr, nullptr, nullptr, p + nx.b[0])
                           : add_tabs(p + mn.b[0], b2(mn), b3(mn), p + mn.gamma, p + mn.beta, p + nx.b[0]);
        if (pieces) so.n_b2pos = b2pos(mn);
        if (S > 1) {
            const MlpOff& nx1 = h->es[1].pe[kn];
            place(so.n[6], p + mn.W[0], 2 * L, PROC_SET1);
            place(so.n[7], p + nx1.W[0], 0, PROC_SET1);
            place(so.n[8], p + nx1.W[0], L, PROC_SET1);
            so.p1_tabs = add_tabs(nullptr, nullptr, nullptr, nullptr, nullptr, p + nx1.b[0]);
        }
    };
    h->steps.assign(c.mps, {});
    for (int k = 0; k < c.mps; ++k) {
        auto& so = h->steps[k];
        for (int q = 0; q < S; ++q) {
            const MlpOff& me = h->es[q].pe[k];
            add_gen(me, true, so.e_gen[q]);
            place_w23(so.e[q][0], so.e[q][1], me, so.e_gen[q], PROC);
            place(so.e[q][2], p + me.W[0], 2 * L, PROC);
            so.e_tabs[q] = add_tabs(nullptr, b2(me), b3(me), p + me.gamma, p + me.beta, nullptr);
            if (pieces) so.e_b2pos[q] = b2pos(me);
        }
        node_side(so, k);
    }
    {
        const MlpOff& m = h->dec;
        place(h->de[0], p + m.W[0], 0, ENDS);
        add_gen(m, false, h->de_gen);                                  // middle layers only: the last one (L -> O) runs on the VALU
        if (nmid > 0) {
            h->de[1].frag = h->de_gen.ch[0];
            place(h->de[1], p + m.W[1], 0, ENDS);
        } else {
            h->de[1] = h->de[0];
        }
        h->de_tabs = add_tabs(p + m.b[0], b2(m), nullptr, nullptr, nullptr, nullptr);
        h->de_w3f = f.size();
        f.resize(f.size() + (size_t)c.O * L);
        for (int o = 0; o < c.O; ++o) pack_tab(f.data() + h->de_w3f + (size_t)o * L, p + m.W[nl - 1] + o, L, c.O);
        h->de_b3 = f.size();
        for (int o = 0; o < c.O; ++o) f.push_back(p[m.b[nl - 1] + o]);
        while (f.size() % 4) f.push_back(0.f);
    }
    // "project only" (mgn_proc_begin) needs step 0's own first layer in the projection slots of some NodeArgs: a dedicated
    // pseudo-step at index mps.  Its fp32 and bf16 copies of the node MLP's chunks (0 .. 3, 6) are step 0's, its fp32 copies of set 0's
    // projection the node encoder's; everything else -- all of its 16-bit pieces -- it builds (tables: bq = b1 of step 0's edge MLP).
    {
        mgn_engine::StepChunks so = h->steps[0];
        for (int i = 0; i < 9; ++i) {
            ChunkRef r;
            if (i < 4 || i == 6) {
                r.frag = so.n[i].frag;
                r.bf = so.n[i].bf;
            }
            so.n[i] = r;
        }
        so.n[4].frag = h->en[2].frag;
        so.n[5].frag = h->en[3].frag;
        node_side(so, c.mps);
        h->steps.push_back(so);
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (sp_size) HIPCHK(h, h->wsp.ensure(sp_size * 2));
    if (bf_size) HIPCHK(h, h->wbf.ensure(bf_size * 2));
    drop_graph(h);
    invalidate_static(h);
    if (f.size() > seg0) small.push_back({seg0, f.size()});
    HIPCHK(h, h->wfrag.ensure(f.size() * 4));
    const float* dp = nullptr;
    if (int rc = dev_params(h, &dp)) return rc;
    HIPCHK(h, h->d_wjobs.ensure(jobs.size() * sizeof(WPackJob)));
    HIPCHK(h, hipMemcpyAsync(h->d_wjobs.p, jobs.data(), jobs.size() * sizeof(WPackJob), hipMemcpyHostToDevice, h->stream));
    for (const auto& sg : small)
        HIPCHK(h, hipMemcpyAsync(h->wfrag.as<float>() + sg.first, f.data() + sg.first, (sg.second - sg.first) * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, launch_pack_weights(L, h->d_wjobs.as<WPackJob>(), (int)jobs.size(), dp, h->wfrag.as<float>(),
                                  h->wsp.as<uint16_t>(), h->wbf.as<uint16_t>(), h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));       // (f and jobs are locals: their copies must have left the host)
    h->wjobs = std::move(jobs);
    h->packed_ok = true;
    return MGN_OK;
}
}  // namespace mgn
extern "C" {

int mgn_get_params(mgn_handle* h, float* packed, size_t n) try {
    if (int rc = need(h, true, false, false)) return rc;
    if (!packed || n != h->params.size()) return fail(h, MGN_E_ARG, "mgn_get_params: size mismatch");
    const float* p = nullptr;
    if (int rc = host_params(h, &p)) return rc;
    memcpy(packed, p, n * sizeof(float));
    return MGN_OK;
} MGN_CATCH(h)

int mgn_set_norms(mgn_handle* h, const float* ns, const float* nsh, const float* es, const float* esh, const float* os,
                  const float* osh) try {
    if (int rc = need(h, false, false)) return rc;
    const mgn_config& c = h->cfg;
    if ((ns == nullptr) != (nsh == nullptr) || (es == nullptr) != (esh == nullptr) || (os == nullptr) != (osh == nullptr))
        return fail(h, MGN_E_ARG, "mgn_set_norms: scale and shift must both be given or both be NULL");
    std::vector<float> v((size_t)2 * (c.Fn + c.Fe + c.O), 0.f);
    float* q = v.data();
    auto put = [&](const float* a, const float* b, int n) {
        for (int i = 0; i < n; ++i) { q[i] = a ? a[i] : 1.f; q[n + i] = b ? b[i] : 0.f; }
        q += 2 * n;
    };
    put(ns, nsh, c.Fn);
    put(es, esh, c.Fe);
    put(os, osh, c.O);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, h->norms.ensure(v.size() * 4));
    HIPCHK(h, hipMemcpy(h->norms.p, v.data(), v.size() * 4, hipMemcpyHostToDevice));
    h->norms_host = v;
    h->norms_host_stale = false;
    invalidate_static(h);
    train_invalidate(h, 4);
    h->have_nnorm = ns != nullptr;
    h->have_enorm = es != nullptr;
    h->have_onorm = os != nullptr;
    return MGN_OK;
} MGN_CATCH(h)

// Node numbering policy of mgn_set_graph (graph_host.h: build_local_graph): 1 = keep the caller's numbering unless the breadth-first
// order of the mesh is RENUMBER_GAIN times more local (DeepMind's trajectories carry arbitrary node numbers and create_base_graph
// passes them through, reference src/graph.jl:30-36; the processor kernels gather sender rows and lose 4-9 % (fp32) / 25 % (bf16)
// on a scattered numbering), 0 = never, 2 = always.  Invisible at the boundary: every array crosses it in the caller's order.
static Switch g_renumber{"MGN_RENUMBER", 1};

// (re)build the local graph from the kept global edge lists and upload it.  keep_owner: node partition unchanged
extern "C++" int mgn::rebuild_graph(mgn_handle* h, int32_t N, const EdgeList* sets, const float* mesh_pos, int32_t pos_dim, bool keep_owner,
                                    const char* who, const int32_t* owner_in, int renumber) {
    shoot_release(h);                     // the companion of mgn_shooting_grad replicates the old graph
    h->have_graph = false;
    h->hx_ready = false;
    h->all_gid.clear();
    invalidate_static(h);
    train_invalidate(h, 2);
    if (!h->host_only) { (void)hipStreamSynchronize(h->stream); drop_graph(h); }
    const std::string why = build_local_graph(N, h->nsets, sets, mesh_pos, pos_dim, owner_in ? owner_in : (keep_owner ? h->g.owner.data() : nullptr),
                                              h->cfg.rank, h->cfg.nranks, h->g,
                                              renumber >= 0 ? renumber : g_renumber);   // (the numbering follows set 0 alone: a later mgn_set_edge_set / mgn_world_edges_dev keeps it)
    if (!why.empty()) return fail(h, MGN_E_ARG, "%s: %s", who, why.c_str());
    const LocalGraph& g = h->g;
    for (int q = 0; q < h->nsets; ++q) h->es[q].ntiles_e = (int32_t)((g.set[q].e_local + TILE - 1) / TILE);
    h->ntiles_n = (g.n_own + TILE - 1) / TILE;
    if (h->host_only) {
        h->have_graph = true;
        return MGN_OK;
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    auto up = [&](DevBuf& d, const void* src, size_t bytes) -> hipError_t {
        hipError_t e = d.ensure(bytes);
        if (e != hipSuccess || bytes == 0) return e;
        return hipMemcpy(d.p, src, bytes, hipMemcpyHostToDevice);
    };
    for (int q = 0; q < h->nsets; ++q) {
        const EdgeTopo& t = g.set[q];
        auto& es = h->es[q];
        HIPCHK(h, up(es.d_snd, t.snd.data(), t.snd.size() * 4));
        HIPCHK(h, up(es.d_rcv, t.rcv.data(), t.rcv.size() * 4));
        HIPCHK(h, up(es.d_rowptr, t.rowptr.data(), t.rowptr.size() * 4));
        HIPCHK(h, up(es.d_edge_gid, t.edge_gid.data(), t.edge_gid.size() * 8));
    }
    HIPCHK(h, up(h->d_own_gid, g.own_gid.data(), g.own_gid.size() * 4));
    HIPCHK(h, up(h->d_send_idx, g.send_idx.data(), g.send_idx.size() * 4));
    return MGN_OK;
}

int mgn_set_graph(mgn_handle* h, int32_t N, int64_t E, const int32_t* senders, const int32_t* receivers, int32_t index_base,
                  const float* mesh_pos, int32_t pos_dim) try {
    if (!h) return MGN_E_ARG;
    if (index_base != 0 && index_base != 1) return fail(h, MGN_E_ARG, "mgn_set_graph: index_base must be 0 or 1");
    if (E < 0 || (E > 0 && (!senders || !receivers))) return fail(h, MGN_E_ARG, "mgn_set_graph: null senders/receivers");
    EdgeList sets[MAX_EDGE_SETS];
    sets[0] = {E, senders, receivers, index_base};
    if (h->nsets > 1) {   // the second set starts empty; keep set 0's global list for the rebuild in mgn_set_edge_set
        h->es[0].gs.assign(senders, senders + E);
        h->es[0].gr.assign(receivers, receivers + E);
        h->es[0].gbase = index_base;
        h->es[1].gs.clear();
        h->es[1].gr.clear();
        h->es[1].have_ef = false;
    }
    if (int rc = rebuild_graph(h, N, sets, mesh_pos, pos_dim, false, "mgn_set_graph")) return rc;
    if (h->host_only) return MGN_OK;
    if (int rc = alloc_latents(h)) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->have_graph = true;
    return MGN_OK;
} MGN_CATCH(h)

// Rank-local ingest (SURVEY.md 8e at scale): what mgn_set_graph computes from the global lists, from the rank's own part of them.
int mgn_partition_nodes(int32_t N, const float* mesh_pos, int32_t pos_dim, int32_t nranks, int32_t* owner) try {
    if (N < 0 || nranks < 1 || (N > 0 && !owner) || (mesh_pos && pos_dim <= 0)) return MGN_E_ARG;
    std::vector<int32_t> o;
    rcb_partition(N, mesh_pos, pos_dim, nranks, o);
    if (N > 0) memcpy(owner, o.data(), (size_t)N * 4);
    return MGN_OK;
} MGN_CATCH(nullptr)

int mgn_set_graph_local(mgn_handle* h, int32_t N, const int32_t* owner, int64_t E_global, int64_t E_touch, const int32_t* senders,
                        const int32_t* receivers, const int64_t* edge_gid, int32_t index_base) try {
    if (!h) return MGN_E_ARG;
    if (h->nsets != 1) return fail(h, MGN_E_UNSUPPORTED, "mgn_set_graph_local: one edge set (a second set is rebuilt from the global lists)");
    if (index_base != 0 && index_base != 1) return fail(h, MGN_E_ARG, "mgn_set_graph_local: index_base must be 0 or 1");
    if (N < 0 || (N > 0 && !owner)) return fail(h, MGN_E_ARG, "mgn_set_graph_local: null owner map");
    if (E_touch < 0 || E_global < E_touch || (E_touch > 0 && (!senders || !receivers || !edge_gid)))
        return fail(h, MGN_E_ARG, "mgn_set_graph_local: null or inconsistent edge arrays");
    for (int32_t i = 0; i < N; ++i)
        if (owner[i] < 0 || owner[i] >= h->cfg.nranks) return fail(h, MGN_E_ARG, "mgn_set_graph_local: owner[%d] = %d outside [0, nranks)", i, owner[i]);
    EdgeList sets[MAX_EDGE_SETS];
    sets[0] = {E_touch, senders, receivers, index_base, edge_gid, E_global};
    if (int rc = rebuild_graph(h, N, sets, nullptr, 0, false, "mgn_set_graph_local", owner)) return rc;
    if (h->host_only) return MGN_OK;
    if (int rc = alloc_latents(h)) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->have_graph = true;
    return MGN_OK;
} MGN_CATCH(h)

int mgn_set_edge_set(mgn_handle* h, int32_t set, int64_t E, const int32_t* senders, const int32_t* receivers, int32_t index_base) try {
    if (!h) return MGN_E_ARG;
    if (!h->have_graph) return fail(h, MGN_E_STATE, "mgn_set_edge_set before mgn_set_graph");
    if (set < 1 || set >= h->nsets) return fail(h, MGN_E_ARG, "mgn_set_edge_set: set %d out of range (handle has %d edge sets; set 0 is mgn_set_graph's)", set, h->nsets);
    if (index_base != 0 && index_base != 1) return fail(h, MGN_E_ARG, "mgn_set_edge_set: index_base must be 0 or 1");
    if (E < 0 || (E > 0 && (!senders || !receivers))) return fail(h, MGN_E_ARG, "mgn_set_edge_set: null senders/receivers");
    auto& e1 = h->es[set];
    e1.gs.assign(senders, senders + E);
    e1.gr.assign(receivers, receivers + E);
    e1.gbase = index_base;
    e1.have_ef = false;
    EdgeList sets[MAX_EDGE_SETS];
    for (int q = 0; q < h->nsets; ++q) sets[q] = {(int64_t)h->es[q].gs.size(), h->es[q].gs.data(), h->es[q].gr.data(), h->es[q].gbase};
    const int32_t n_halo_before = h->g.n_halo;
    if (int rc = rebuild_graph(h, h->g.N, sets, nullptr, 0, true, "mgn_set_edge_set")) return rc;
    if (h->host_only) return MGN_OK;
    // node numbering is unchanged with one partition (no boundary / halo): V and set 0's latents stay valid and only the
    // new set's buffers are (re)sized; a changed halo re-sizes everything that is indexed by owned + halo rows
    if (h->cfg.nranks == 1 && n_halo_before == 0) {
        if (int rc = alloc_edge_set(h, set)) return rc;
    } else if (int rc = alloc_latents(h)) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->have_graph = true;
    return MGN_OK;
} MGN_CATCH(h)

int mgn_edge_set_info(const mgn_handle* h, int32_t set, int64_t* E, int64_t* e_local) try {
    if (!h || !h->have_graph) return MGN_E_STATE;
    if (set < 0 || set >= h->nsets) return MGN_E_ARG;
    if (E) *E = h->g.set[set].E;
    if (e_local) *e_local = h->g.set[set].e_local;
    return MGN_OK;
} MGN_CATCH(nullptr)

int mgn_set_edge_features(mgn_handle* h, int32_t set, const float* ef) try {
    if (int rc = need(h, false, true)) return rc;
    if (set < 1 || set >= h->nsets) return fail(h, MGN_E_ARG, "mgn_set_edge_features: set %d out of range", set);
    auto& es = h->es[set];
    const size_t bytes = (size_t)h->g.set[set].E * es.Fe * 4;
    if (bytes && !ef) return fail(h, MGN_E_ARG, "mgn_set_edge_features: null input");
    const void* before = es.d_ef.p;
    HIPCHK(h, es.d_ef.ensure(bytes));
    if (es.d_ef.p != before && h->fwd_exec) {   // the captured forward reads this buffer
        (void)hipStreamSynchronize(h->stream);
        (void)hipGraphExecDestroy(h->fwd_exec);
        h->fwd_exec = nullptr;
        h->fwd_warm = false;
    }
    if (bytes) HIPCHK(h, hipMemcpyAsync(es.d_ef.p, ef, bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    es.have_ef = true;
    return MGN_OK;
} MGN_CATCH(h)

int mgn_partition_info(const mgn_handle* h, int32_t* n_own, int32_t* n_halo, int64_t* e_local) try {
    if (!h || !h->have_graph) return MGN_E_STATE;
    if (n_own) *n_own = h->g.n_own;
    if (n_halo) *n_halo = h->g.n_halo;
    if (e_local) *e_local = h->g.set[0].e_local;
    return MGN_OK;
} MGN_CATCH(nullptr)

int mgn_owned_nodes(const mgn_handle* h, int32_t* ids) try {
    if (!h || !h->have_graph || !ids) return MGN_E_STATE;
    memcpy(ids, h->g.own_gid.data(), h->g.own_gid.size() * 4);
    return MGN_OK;
} MGN_CATCH(nullptr)

int mgn_local_edges(const mgn_handle* h, int64_t* ids) try {
    if (!h || !h->have_graph || !ids) return MGN_E_STATE;
    memcpy(ids, h->g.set[0].edge_gid.data(), h->g.set[0].edge_gid.size() * 8);
    return MGN_OK;
} MGN_CATCH(nullptr)

int mgn_halo_counts(const mgn_handle* h, int32_t* send_rows, int32_t* recv_rows) try {
    if (!h || !h->have_graph) return MGN_E_STATE;
    for (int q = 0; q < h->cfg.nranks; ++q) {
        if (send_rows) send_rows[q] = h->g.send_rows[q];
        if (recv_rows) recv_rows[q] = h->g.recv_rows[q];
    }
    return MGN_OK;
} MGN_CATCH(nullptr)

int mgn_halo_nodes(const mgn_handle* h, int32_t* ids) try {
    if (!h || !h->have_graph || !ids) return MGN_E_STATE;
    memcpy(ids, h->g.halo_gid.data(), h->g.halo_gid.size() * 4);
    return MGN_OK;
} MGN_CATCH(nullptr)

int mgn_halo_send_index(const mgn_handle* h, int32_t* rows) try {
    if (!h || !h->have_graph || !rows) return MGN_E_STATE;
    memcpy(rows, h->g.send_idx.data(), h->g.send_idx.size() * 4);
    return MGN_OK;
} MGN_CATCH(nullptr)

int mgn_local_graph(const mgn_handle* h, int32_t* snd, int32_t* rcv, int32_t* rowptr) try {
    if (!h || !h->have_graph) return MGN_E_STATE;
    if (snd) memcpy(snd, h->g.set[0].snd.data(), h->g.set[0].snd.size() * 4);
    if (rcv) memcpy(rcv, h->g.set[0].rcv.data(), h->g.set[0].rcv.size() * 4);
    if (rowptr) memcpy(rowptr, h->g.set[0].rowptr.data(), h->g.set[0].rowptr.size() * 4);
    return MGN_OK;
} MGN_CATCH(nullptr)

int mgn_node_owner(const mgn_handle* h, int32_t* owner) try {
    if (!h || !h->have_graph || !owner) return MGN_E_STATE;
    memcpy(owner, h->g.owner.data(), h->g.owner.size() * 4);
    return MGN_OK;
} MGN_CATCH(nullptr)

int mgn_boundary_count(const mgn_handle* h, int32_t* n_boundary) try {
    if (!h || !h->have_graph || !n_boundary) return MGN_E_STATE;
    *n_boundary = h->g.n_boundary;
    return MGN_OK;
} MGN_CATCH(nullptr)

// ---- staged pipeline ----------------------------------------------------------------------------
// engine_order: the node rows must sit on the device in the ENGINE's order even on one partition -- the callers that later overwrite
// the state slot of d_nfA with rows in that order (mgn_set_static + mgn_ode_step(x), mgn_rollout)
extern "C++" int mgn::upload_inputs(mgn_handle* h, const float* a, int wa, const float* b, int wb, const float* ef, bool engine_order) {
    const LocalGraph& g = h->g;
    h->in_wa = wa;
    h->in_wb = wb;
    if (h->cfg.nranks > 1 || (engine_order && g.renumbered)) {
        // a partition needs 1 / nranks of the inputs: gather the owned node rows and the local edge rows on the host and
        // upload those (M-1M on 8 GPUs: 13 MB instead of 108 MB per rank and forward); the encoders then read them in
        // local order (null gid).  (A renumbered SINGLE partition, graph_host.h, uploads the caller's arrays as they are for
        // mgn_forward and the one-shot mgn_ode_step -- one contiguous copy each -- and the encoders gather through own_gid / edge_gid on
        // the device: a host gather of 6 M edge rows costs tens of ms per forward.  Where the state is kept in the engine's order
        // (engine_order), it goes the partitions' way.)
        h->in_local = true;
        const EdgeTopo& t = g.set[0];
        const int Fe = h->cfg.Fe;
        std::vector<float> loc((size_t)g.n_own * (wa + wb) + (size_t)t.e_local * Fe);
        float* la = loc.data();
        float* lb = la + (size_t)g.n_own * wa;
        float* le = lb + (size_t)g.n_own * wb;
        for (int32_t i = 0; i < g.n_own; ++i) {
            memcpy(la + (size_t)i * wa, a + (size_t)g.own_gid[i] * wa, (size_t)wa * 4);
            if (wb > 0) memcpy(lb + (size_t)i * wb, b + (size_t)g.own_gid[i] * wb, (size_t)wb * 4);
        }
        for (int64_t j = 0; j < t.e_local; ++j) memcpy(le + (size_t)j * Fe, ef + (size_t)t.edge_gid[j] * Fe, (size_t)Fe * 4);
        HIPCHK(h, h->d_nfA.ensure((size_t)g.n_own * wa * 4));
        HIPCHK(h, h->d_nfB.ensure((size_t)g.n_own * (wb > 0 ? wb : 1) * 4));
        HIPCHK(h, h->es[0].d_ef.ensure((size_t)t.e_local * Fe * 4));
        HIPCHK(h, hipMemcpyAsync(h->d_nfA.p, la, (size_t)g.n_own * wa * 4, hipMemcpyHostToDevice, h->stream));
        if (wb > 0) HIPCHK(h, hipMemcpyAsync(h->d_nfB.p, lb, (size_t)g.n_own * wb * 4, hipMemcpyHostToDevice, h->stream));
        if (t.e_local > 0) HIPCHK(h, hipMemcpyAsync(h->es[0].d_ef.p, le, (size_t)t.e_local * Fe * 4, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));   // `loc` goes out of scope
        return MGN_OK;
    }
    h->in_local = false;
    HIPCHK(h, h->d_nfA.ensure((size_t)g.N * wa * 4));
    HIPCHK(h, hipMemcpyAsync(h->d_nfA.p, a, (size_t)g.N * wa * 4, hipMemcpyHostToDevice, h->stream));
    if (wb > 0) {
        HIPCHK(h, h->d_nfB.ensure((size_t)g.N * wb * 4));
        HIPCHK(h, hipMemcpyAsync(h->d_nfB.p, b, (size_t)g.N * wb * 4, hipMemcpyHostToDevice, h->stream));
    }
    HIPCHK(h, h->es[0].d_ef.ensure((size_t)g.set[0].E * h->cfg.Fe * 4));
    HIPCHK(h, hipMemcpyAsync(h->es[0].d_ef.p, ef, (size_t)g.set[0].E * h->cfg.Fe * 4, hipMemcpyHostToDevice, h->stream));
    return MGN_OK;
}

int mgn_fwd_upload(mgn_handle* h, const float* nf, const float* ef) try {
    if (int rc = need(h, false, true)) return rc;
    invalidate_static(h);
    if (!nf || (!ef && h->g.set[0].E > 0)) return fail(h, MGN_E_ARG, "mgn_fwd_upload: null input");
    return upload_inputs(h, nf, h->cfg.Fn, nullptr, 0, ef);
} MGN_CATCH(h)

static int project_set(mgn_handle* h, int k, int q, int32_t tile0 = 0, int32_t ntiles = -1) {   // P,Q of set q for step k (k = mps: step 0)
    if (ntiles < 0) ntiles = h->ntiles_n;
    if (bf16_pipe(h)) {
        BfNodeArgs b = bf_node_args(h, k, q, true);
        b.tile0 = tile0;
        b.ntiles = ntiles;
        HIPCHK(h, launch_project_bf16(b, h->stream));
        return MGN_OK;
    }
    NodeArgs a = node_args(h, k, 2, q);
    a.tile0 = tile0;
    a.ntiles = ntiles;
    HIPCHK(h, launch_project(h->cfg.L, a, h->stream));
    return MGN_OK;
}

extern "C++" int mgn::encode_impl(mgn_handle* h, bool use_norms, bool nodes, bool edges) {
    const mgn_config& c = h->cfg;
    const LocalGraph& g = h->g;
    const float* nrm = h->norms.as<float>();
    ProfScope ps(h, F_ENC);
    if (nodes) {
        EncNodeArgs a{};
        a.n = g.n_own;
        a.ntiles = h->ntiles_n;
        a.gid = h->in_local ? nullptr : h->d_own_gid.as<int32_t>();
        a.srcA = h->srcA_override ? h->srcA_override : h->d_nfA.as<float>();
        a.wa = h->in_wa;
        a.srcB = h->d_nfB.as<float>();
        a.wb = h->in_wb;
        if (use_norms && h->have_nnorm) { a.scale = nrm; a.shift = nrm + c.Fn; }
        a.w1f = W(h, h->en_w1f);
        a.V = h->V.as<float>();
        a.P = h->es[0].P.as<float>();
        a.Q = h->es[0].Q.as<float>();
        a.w = stage_weights(h, h->en, h->en_tabs, h->en_gen, true);
        HIPCHK(h, launch_enc_node(c.L, a, h->stream));
        if (is_bf16(h)) {   // fp32 encoder output -> bf16 state; P,Q of step 0 from the bf16 latents
            HIPCHK(h, launch_tile_f32_to_bf16(h->V.as<float>(), h->bV.as<uint16_t>(), h->ntiles_n, h->stream));
            if (int rc = project_set(h, c.mps, 0)) return rc;
        }
        for (int q = 1; q < h->nsets; ++q)
            if (int rc = project_set(h, c.mps, q)) return rc;
    }
    if (edges) {
        for (int q = 0; q < h->nsets; ++q) {
            auto& es = h->es[q];
            EncEdgeArgs b{};
            b.E = g.set[q].e_local;
            b.ntiles = es.ntiles_e;
            b.gid = (q == 0 && h->in_local) ? nullptr : es.d_edge_gid.as<int64_t>();
            b.ef = es.d_ef.as<float>();
            b.Fe = es.Fe;
            if (q == 0 && use_norms && h->have_enorm) { b.scale = nrm + 2 * c.Fn; b.shift = nrm + 2 * c.Fn + c.Fe; }
            b.w1f = W(h, es.ee_w1f);
            b.Elat = es.Elat.as<float>();
            b.w = stage_weights(h, es.ee, es.ee_tabs, es.ee_gen, true);
            HIPCHK(h, launch_enc_edge(c.L, b, h->stream));
            if (is_bf16(h)) HIPCHK(h, launch_tile_f32_to_bf16(es.Elat.as<float>(), es.bElat.as<uint16_t>(), es.ntiles_e, h->stream));
        }
    }
    return MGN_OK;
}

static int need_set_features(mgn_handle* h) {
    for (int q = 1; q < h->nsets; ++q)
        if (h->g.set[q].E > 0 && !h->es[q].have_ef)
            return fail(h, MGN_E_STATE, "edge set %d has edges but no features: call mgn_set_edge_features after mgn_set_edge_set", q);
    return MGN_OK;
}

int mgn_fwd_encode(mgn_handle* h) try {
    if (int rc = need(h, true, true)) return rc;
    if (!h->d_nfA.p) return fail(h, MGN_E_STATE, "mgn_fwd_encode before mgn_fwd_upload");
    if (int rc = need_set_features(h)) return rc;
    return encode_impl(h, false);
} MGN_CATCH(h)

int mgn_proc_begin(mgn_handle* h) try {
    if (int rc = need(h, true, true)) return rc;
    ProfScope ps(h, F_NODE);
    for (int q = 0; q < h->nsets; ++q)
        if (int rc = project_set(h, h->cfg.mps, q)) return rc;
    return MGN_OK;
} MGN_CATCH(h)

static int proc_edge_range(mgn_handle* h, int32_t k, int32_t phase) {   // phase 0: all tiles, 1: interior tiles, 2: boundary tiles
    bool work = false;
    for (int q = 0; q < h->nsets; ++q) {
        const int32_t tb = boundary_tiles(h, q), nt = h->es[q].ntiles_e;
        work = work || (phase == 0 ? nt : (phase == 1 ? nt - tb : tb)) > 0;
    }
    if (!work) return MGN_OK;
    ProfScope ps(h, phase == 2 ? F_EDGE_BND : F_EDGE);
    for (int q = 0; q < h->nsets; ++q) {
        const int32_t tb = boundary_tiles(h, q), nt = h->es[q].ntiles_e;
        const int32_t t0 = phase == 1 ? tb : 0, n = phase == 0 ? nt : (phase == 1 ? nt - tb : tb);
        if (n <= 0) continue;
        if (bf16_pipe(h)) {
            BfEdgeArgs a = bf_edge_args(h, k, q);
            a.tile0 = t0;
            a.ntiles = n;
            HIPCHK(h, launch_edge_bf16(a, h->stream));
        } else {
            EdgeArgs a = edge_args(h, k, q);
            a.tile0 = t0;
            a.ntiles = n;
            HIPCHK(h, launch_edge_step(h->cfg.L, a, h->stream));
        }
    }
    return MGN_OK;
}

int mgn_proc_edge(mgn_handle* h, int32_t k) try {
    if (int rc = need(h, true, true)) return rc;
    if (k < 0 || k >= h->cfg.mps) return fail(h, MGN_E_ARG, "mgn_proc_edge: step %d out of range", k);
    return proc_edge_range(h, k, 0);
} MGN_CATCH(h)

int mgn_proc_edge_phase(mgn_handle* h, int32_t k, int32_t phase) try {
    if (int rc = need(h, true, true)) return rc;
    if (k < 0 || k >= h->cfg.mps) return fail(h, MGN_E_ARG, "mgn_proc_edge_phase: step %d out of range", k);
    if (phase != 1 && phase != 2) return fail(h, MGN_E_ARG, "mgn_proc_edge_phase: phase must be 1 or 2");
    return proc_edge_range(h, k, phase);
} MGN_CATCH(h)

int mgn_edge_boundary_tiles(const mgn_handle* h, int32_t set, int32_t* boundary, int32_t* total) try {
    if (!h || !h->have_graph) return MGN_E_STATE;
    if (set < 0 || set >= h->nsets) return MGN_E_ARG;
    if (boundary) *boundary = boundary_tiles(h, set);
    if (total) *total = h->es[set].ntiles_e;
    return MGN_OK;
} MGN_CATCH(nullptr)

// the node MLP of step k and, with project_next, P / Q of step k + 1 for every edge set: in the MLP's launch where the kernels have
// that form at this size (kernels.hip: node_step_projects), else one projection launch per set behind it
static int node_side(mgn_handle* h, int32_t k, bool project_next) {
    bool projected = false;
    if (bf16_pipe(h)) {
        HIPCHK(h, launch_node_bf16(bf_node_args(h, k), h->stream));
    } else {
        NodeArgs a = node_args(h, k, project_next ? 1 : 0);
        projected = project_next && node_step_projects(h->cfg.L, a);
        a.mode = projected ? 1 : 0;      // (the mode is all that differs between the two argument blocks)
        HIPCHK(h, launch_node_step(h->cfg.L, a, h->stream));
    }
    for (int q = 0; project_next && !projected && q < h->nsets; ++q)
        if (int rc = project_set(h, k, q)) return rc;
    return MGN_OK;
}

int mgn_proc_node(mgn_handle* h, int32_t k, int32_t project_next) try {
    if (int rc = need(h, true, true)) return rc;
    if (k < 0 || k >= h->cfg.mps) return fail(h, MGN_E_ARG, "mgn_proc_node: step %d out of range", k);
    if (project_next && k + 1 >= h->cfg.mps) return fail(h, MGN_E_ARG, "mgn_proc_node: no step %d to project for", k + 1);
    ProfScope ps(h, F_NODE);
    return node_side(h, k, project_next != 0);
} MGN_CATCH(h)

int mgn_proc_node_phase(mgn_handle* h, int32_t k, int32_t phase) try {
    if (int rc = need(h, true, true)) return rc;
    if (k < -1 || k + 1 >= h->cfg.mps) return fail(h, MGN_E_ARG, "mgn_proc_node_phase: no step %d to project for", k + 1);
    if (phase != 1 && phase != 2) return fail(h, MGN_E_ARG, "mgn_proc_node_phase: phase must be 1 or 2");
    ProfScope ps(h, F_NODE);
    const int ntb_all = (h->g.n_boundary + TILE - 1) / TILE;   // tiles that contain a boundary node
    const int ntb = ntb_all < h->ntiles_n ? ntb_all : h->ntiles_n;
    if (phase == 1 && k >= 0)
        if (int rc = node_side(h, k, false)) return rc;
    const int32_t tile0 = phase == 1 ? 0 : ntb, nt = phase == 1 ? ntb : h->ntiles_n - ntb;
    for (int q = 0; q < h->nsets; ++q)
        if (int rc = project_set(h, k >= 0 ? k : h->cfg.mps, q, tile0, nt)) return rc;
    return MGN_OK;
} MGN_CATCH(h)

extern "C++" int mgn::decode_impl(mgn_handle* h, bool use_norms) {
    const mgn_config& c = h->cfg;
    ProfScope ps(h, F_DEC);
    if (is_bf16(h)) HIPCHK(h, launch_tile_bf16_to_f32(h->bV.as<uint16_t>(), h->V.as<float>(), h->ntiles_n, h->stream));
    DecArgs a{};
    a.n = h->g.n_own;
    a.ntiles = h->ntiles_n;
    a.V = h->V.as<float>();
    a.w3f = W(h, h->de_w3f);
    a.b3 = W(h, h->de_b3);
    a.O = c.O;
    if (use_norms && h->have_onorm) {
        const float* nrm = h->norms.as<float>() + 2 * c.Fn + 2 * c.Fe;
        a.oscale = nrm;
        a.oshift = nrm + c.O;
    }
    a.mask = (use_norms && h->have_mask) ? h->d_mask.as<float>() : nullptr;
    a.gid = h->d_own_gid.as<int32_t>();
    a.out = h->out_override ? h->out_override : h->d_out.as<float>();
    a.w = stage_weights(h, h->de, h->de_tabs, h->de_gen, false);
    HIPCHK(h, launch_decode(c.L, a, h->stream));
    return MGN_OK;
}

int mgn_fwd_decode(mgn_handle* h) try {
    if (int rc = need(h, true, true)) return rc;
    return decode_impl(h, false);
} MGN_CATCH(h)

int mgn_fwd_download(mgn_handle* h, float* out) try {
    if (int rc = need(h, false, true)) return rc;
    if (!out) return fail(h, MGN_E_ARG, "mgn_fwd_download: null out");
    const LocalGraph& g = h->g;
    const int O = h->cfg.O;
    std::vector<float> loc((size_t)g.n_own * O);
    HIPCHK(h, hipMemcpyAsync(loc.data(), h->d_out.p, loc.size() * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int32_t i = 0; i < g.n_own; ++i) memcpy(out + (size_t)g.own_gid[i] * O, loc.data() + (size_t)i * O, (size_t)O * 4);
    return MGN_OK;
} MGN_CATCH(h)

static int forward_partitioned(mgn_handle* h, const float* nf, const float* ef, float* out);
static int processor_pass_staged(mgn_handle* h, int32_t nsteps, bool begin);

// the O x N state of a right-hand side: one partition takes it as it is, a partitioned handle the rows it owns
static int upload_state(mgn_handle* h, const float* x) {
    const LocalGraph& g = h->g;
    const int O = h->cfg.O;
    if (h->cfg.nranks == 1 && !g.renumbered) {
        HIPCHK(h, hipMemcpyAsync(h->d_nfA.p, x, (size_t)g.N * O * 4, hipMemcpyHostToDevice, h->stream));
        return MGN_OK;
    }
    std::vector<float> loc((size_t)g.n_own * O);
    for (int32_t i = 0; i < g.n_own; ++i) memcpy(loc.data() + (size_t)i * O, x + (size_t)g.own_gid[i] * O, (size_t)O * 4);
    HIPCHK(h, hipMemcpyAsync(h->d_nfA.p, loc.data(), loc.size() * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return MGN_OK;
}

extern "C++" int mgn::run_processor(mgn_handle* h, int nsteps) {
    // partitioned: the staged schedule; P, Q of step 0 came from the encoder, so the pass starts with their exchange
    if (h->cfg.nranks != 1) return processor_pass_staged(h, nsteps, false);
    for (int k = 0; k < nsteps; ++k) {
        if (int rc = mgn_proc_edge(h, k)) return rc;
        if (int rc = mgn_proc_node(h, k, k + 1 < nsteps ? 1 : 0)) return rc;
    }
    return MGN_OK;
}

int mgn_forward(mgn_handle* h, const float* nf, const float* ef, float* out) try {
    if (h && !h->host_only && h->cfg.ln_dims == MGN_LN_ALL) return lnall_forward(h, nf, ef, out);
    if (int rc = need(h, true, true)) return rc;
    if (h->cfg.nranks != 1) return forward_partitioned(h, nf, ef, out);
    if (int rc = need_set_features(h)) return rc;
    const float* nfA_before = h->d_nfA.as<float>();
    const float* ef_before = h->es[0].d_ef.as<float>();
    const int wa_before = h->in_wa, wb_before = h->in_wb;
    if (int rc = mgn_fwd_upload(h, nf, ef)) return rc;
    if (h->fwd_exec && (nfA_before != h->d_nfA.as<float>() || ef_before != h->es[0].d_ef.as<float>() || wa_before != h->in_wa || wb_before != h->in_wb)) {
        (void)hipGraphExecDestroy(h->fwd_exec);   // an input buffer moved or changed its layout since the capture
        h->fwd_exec = nullptr;
        h->fwd_warm = false;
    }
    auto launches = [&]() -> int {
        if (int rc = encode_impl(h, false)) return rc;
        if (int rc = run_processor(h, h->cfg.mps)) return rc;
        return decode_impl(h, false);
    };
    if (int rc = run_graphed(h, h->stream, small_graphable(h), h->fwd_exec, h->fwd_warm, launches)) return rc;
    return mgn_fwd_download(h, out);
} MGN_CATCH(h)

int mgn_set_static(mgn_handle* h, const float* onehot, const float* ef_raw, const float* val_mask) try {
    const bool lnall = h && h->cfg.ln_dims == MGN_LN_ALL;
    if (int rc = need(h, true, true, !lnall, true)) return rc;
    const mgn_config& c = h->cfg;
    if (c.nranks != 1) if (int rc = need_comm(h, "mgn_set_static")) return rc;
    if (h->nsets != 1) return fail(h, MGN_E_STATE, "mgn_set_static / mgn_ode_step / mgn_rollout mirror the reference's single-edge-set RHS (src/solve.jl:188-219)");
    if (!ef_raw || (c.Fn > c.O && !onehot)) return fail(h, MGN_E_ARG, "mgn_set_static: null argument");
    if (c.Fn < c.O) return fail(h, MGN_E_ARG, "mgn_set_static: Fn < O");
    const LocalGraph& g = h->g;
    invalidate_static(h);
    {   // static inputs through the common upload (a partitioned handle keeps the rows it owns); the state slot is a placeholder
        std::vector<float> x0((size_t)g.N * c.O, 0.f);
        if (int rc = upload_inputs(h, x0.data(), c.O, onehot, c.Fn - c.O, ef_raw, true)) return rc;
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    h->have_mask = val_mask != nullptr;
    if (val_mask) {
        HIPCHK(h, h->d_mask.ensure((size_t)g.N * 4));
        HIPCHK(h, hipMemcpyAsync(h->d_mask.p, val_mask, (size_t)g.N * 4, hipMemcpyHostToDevice, h->stream));
    }
    if (lnall) {   // whole-array LayerNorm: the unfused right-hand side (mgn_train.cpp) encodes the edges on its first evaluation
        if (int rc = lnall_rhs_prepare(h)) return rc;
        HIPCHK(h, hipStreamSynchronize(h->stream));
        h->have_static = true;
        return MGN_OK;
    }
    if (int rc = encode_impl(h, true, false, true)) return rc;       // edge encoder: once per trajectory
    const bool bf = is_bf16(h);
    const size_t eb = tile_floats(h->es[0].ntiles_e, c.L) * (bf ? 2 : 4);
    HIPCHK(h, h->es[0].elat0.ensure(eb));
    HIPCHK(h, hipMemcpyAsync(h->es[0].elat0.p, bf ? h->es[0].bElat.p : h->es[0].Elat.p, eb, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->have_static = true;
    return MGN_OK;
} MGN_CATCH(h)

// ode_step under ln_dims = MGN_LN_ALL: build_graph's normalisation on the host, the unfused whole-array forward, inverse_data and
// val_mask on the host (reference src/graph.jl:80-93, src/solve.jl:198-218).  The one-shot form only; a hedge, not a fast path.
static int lnall_ode_step(mgn_handle* h, const float* x, const float* onehot, const float* ef_raw, const float* val_mask, float* dxdt) {
    const mgn_config& c = h->cfg;
    if (!h->have_params) return fail(h, MGN_E_STATE, "mgn_set_params has not been called");
    if (!h->have_graph) return fail(h, MGN_E_STATE, "mgn_set_graph has not been called");
    if (!x || !dxdt) return fail(h, MGN_E_ARG, "mgn_ode_step: null argument");
    if (c.Fn < c.O) return fail(h, MGN_E_ARG, "mgn_ode_step: Fn < O");
    if (!onehot && !ef_raw && !val_mask) {   // resident form: static inputs from mgn_set_static, only the state moves
        if (!h->have_static) return fail(h, MGN_E_STATE, "mgn_ode_step without static inputs: call mgn_set_static first or pass them");
        if (int rc = upload_state(h, x)) return rc;
        if (int rc = lnall_rhs_prepare(h)) return rc;
        HIPCHK(h, h->d_out.ensure((size_t)(h->g.n_own > 0 ? h->g.n_own : 1) * c.O * 4));
        if (!h->lnall_edges) {        // first evaluation of the trajectory: the edge encoder runs too (eager)
            if (int rc = lnall_rhs_dev(h, h->d_nfA.as<float>(), h->d_out.as<float>(), false)) return rc;
            h->lnall_edges = true;
        } else {                      // afterwards the ~130 launches of a right-hand side replay from one launch graph (small meshes)
            auto launches = [&]() -> int { return lnall_rhs_dev(h, h->d_nfA.as<float>(), h->d_out.as<float>(), true); };
            if (int rc = run_graphed(h, h->stream, small_graphable(h), h->rhs_exec, h->rhs_warm, launches)) return rc;
        }
        return mgn_fwd_download(h, dxdt);
    }
    if (!ef_raw || (c.Fn > c.O && !onehot)) return fail(h, MGN_E_ARG, "mgn_ode_step: null argument");
    invalidate_static(h);   // the one-shot path overwrites the resident inputs
    if (int rc = sync_norms_host(h)) return rc;
    const int64_t N = h->g.N, E = h->g.set[0].E;
    const float* nrm = h->norms_host.empty() ? nullptr : h->norms_host.data();   // [node scale, shift | edge scale, shift | out scale, shift]
    const float* ns = (nrm && h->have_nnorm) ? nrm : nullptr;
    const float* es = (nrm && h->have_enorm) ? nrm + 2 * c.Fn : nullptr;
    const float* os = (nrm && h->have_onorm) ? nrm + 2 * c.Fn + 2 * c.Fe : nullptr;
    std::vector<float> nf((size_t)N * c.Fn), ef((size_t)E * c.Fe), out((size_t)N * c.O);
    const int W1 = c.Fn - c.O;
    for (int64_t n = 0; n < N; ++n)
        for (int f = 0; f < c.Fn; ++f) {
            const float v = f < c.O ? x[n * c.O + f] : onehot[n * W1 + (f - c.O)];
            nf[(size_t)n * c.Fn + f] = ns ? v * ns[f] + ns[c.Fn + f] : v;
        }
    for (int64_t j = 0; j < E; ++j)
        for (int f = 0; f < c.Fe; ++f) ef[(size_t)j * c.Fe + f] = es ? ef_raw[j * c.Fe + f] * es[f] + es[c.Fe + f] : ef_raw[j * c.Fe + f];
    if (int rc = lnall_forward(h, nf.data(), ef.data(), out.data())) return rc;
    for (int64_t n = 0; n < N; ++n)
        for (int o = 0; o < c.O; ++o) {
            const float y = os ? out[(size_t)n * c.O + o] * os[o] + os[c.O + o] : out[(size_t)n * c.O + o];
            dxdt[n * c.O + o] = val_mask ? y * val_mask[n] : y;
        }
    return MGN_OK;
}

int mgn_ode_step(mgn_handle* h, const float* x, const float* onehot, const float* ef_raw, const float* val_mask, float* dxdt) try {
    if (h && !h->host_only && h->cfg.ln_dims == MGN_LN_ALL) return lnall_ode_step(h, x, onehot, ef_raw, val_mask, dxdt);
    if (int rc = need(h, true, true)) return rc;
    const mgn_config& c = h->cfg;
    if (h->cfg.nranks != 1) if (int rc = need_comm(h, "mgn_ode_step")) return rc;
    if (h->nsets != 1) return fail(h, MGN_E_STATE, "%s mirrors the reference's single-edge-set RHS (src/solve.jl:188-219); this handle has two edge sets", "mgn_ode_step");
    if (!x || !dxdt) return fail(h, MGN_E_ARG, "mgn_ode_step: null argument");
    if (c.Fn < c.O) return fail(h, MGN_E_ARG, "mgn_ode_step: Fn < O");
    if (!onehot && !ef_raw && !val_mask) {
        // fast path: static inputs and encoded edges are resident (mgn_set_static); only the state moves
        if (!h->have_static) return fail(h, MGN_E_STATE, "mgn_ode_step without static inputs: call mgn_set_static first or pass them");
        if (int rc = upload_state(h, x)) return rc;
        auto launches = [&]() -> int {
            if (int rc = encode_impl(h, true, true, false)) return rc;
            const bool bf = is_bf16(h);
            const size_t eb = tile_floats(h->es[0].ntiles_e, c.L) * (bf ? 2 : 4);
            if (elat_src_ok(h)) h->elat_src_override = h->es[0].elat0.as<float>();
            else HIPCHK(h, hipMemcpyAsync(bf ? h->es[0].bElat.p : h->es[0].Elat.p, h->es[0].elat0.p, eb, hipMemcpyDeviceToDevice, h->stream));
            const int rcp = run_processor(h, c.mps);
            h->elat_src_override = nullptr;
            if (rcp) return rcp;
            return decode_impl(h, true);
        };
        // a Julia-driven solve calls this once per right-hand side
        if (c.nranks != 1) {        // (no hipGraph around communicator calls)
            if (int rc = launches()) return rc;
            return gather_rows_global(h, h->d_out.as<float>(), c.O, dxdt);
        }
        if (int rc = run_graphed(h, h->stream, small_graphable(h), h->rhs_exec, h->rhs_warm, launches)) return rc;
        return mgn_fwd_download(h, dxdt);
    }
    if (!ef_raw || (c.Fn > c.O && !onehot)) return fail(h, MGN_E_ARG, "mgn_ode_step: null argument");
    invalidate_static(h);   // the one-shot path overwrites the resident inputs
    if (int rc = upload_inputs(h, x, c.O, onehot, c.Fn - c.O, ef_raw)) return rc;
    h->have_mask = val_mask != nullptr;
    if (val_mask) {
        HIPCHK(h, h->d_mask.ensure((size_t)h->g.N * 4));
        HIPCHK(h, hipMemcpyAsync(h->d_mask.p, val_mask, (size_t)h->g.N * 4, hipMemcpyHostToDevice, h->stream));
    }
    if (int rc = encode_impl(h, true)) return rc;
    if (int rc = run_processor(h, c.mps)) return rc;
    if (int rc = decode_impl(h, true)) return rc;
    if (c.nranks != 1) return gather_rows_global(h, h->d_out.as<float>(), c.O, dxdt);    // the complete dx/dt on every rank
    return mgn_fwd_download(h, dxdt);
} MGN_CATCH(h)

// ---- latents -------------------------------------------------------------------------------------
// Host boundary of the latents: the caller's arrays travel over PCIe as they are (one contiguous copy each) and
// the gather into engine order / tile-major storage runs on the device.
static int import_edges(mgn_handle* h, int q, const float* e) {
    const EdgeTopo& t = h->g.set[q];
    auto& es = h->es[q];
    const int L = h->cfg.L;
    if (t.e_local > 0) {
        if (!e) return fail(h, MGN_E_ARG, "latents import: null edge input");
        const size_t ebytes = (size_t)t.E * L * 4;
        HIPCHK(h, h->stage.ensure(ebytes));
        HIPCHK(h, hipMemcpyAsync(h->stage.p, e, ebytes, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, launch_rows_to_tiles(h->stage.as<float>(), es.d_edge_gid.as<int64_t>(), nullptr, es.Elat.as<float>(), t.e_local, L, h->stream));
    }
    // bf16 mode: the processor state proper is the bf16 copy (rounded once, on the device)
    if (is_bf16(h)) HIPCHK(h, launch_tile_f32_to_bf16(es.Elat.as<float>(), es.bElat.as<uint16_t>(), es.ntiles_e, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return MGN_OK;
}

static int export_edges(mgn_handle* h, int q, float* e) {
    const EdgeTopo& t = h->g.set[q];
    auto& es = h->es[q];
    const int L = h->cfg.L;
    if (!e || t.E == 0) return MGN_OK;
    if (is_bf16(h)) HIPCHK(h, launch_tile_bf16_to_f32(es.bElat.as<uint16_t>(), es.Elat.as<float>(), es.ntiles_e, h->stream));
    const size_t ebytes = (size_t)t.E * L * 4;
    HIPCHK(h, h->stage.ensure(ebytes));
    // single partition: every row is owned, the staging image is complete; else keep the caller's foreign rows
    if (h->cfg.nranks != 1) HIPCHK(h, hipMemcpyAsync(h->stage.p, e, ebytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, launch_tiles_to_rows(es.Elat.as<float>(), es.d_edge_gid.as<int64_t>(), nullptr, h->stage.as<float>(), t.e_local, L, h->stream));
    HIPCHK(h, hipMemcpyAsync(e, h->stage.p, ebytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return MGN_OK;
}

int mgn_latents_import(mgn_handle* h, const float* v, const float* e) try {
    if (int rc = need(h, false, true)) return rc;
    if (!v) return fail(h, MGN_E_ARG, "mgn_latents_import: null input");
    const LocalGraph& g = h->g;
    const int L = h->cfg.L;
    const size_t vb = (size_t)g.N * L * 4;
    HIPCHK(h, h->stage.ensure(vb));
    HIPCHK(h, hipMemcpyAsync(h->stage.p, v, vb, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, launch_rows_to_tiles(h->stage.as<float>(), nullptr, h->d_own_gid.as<int32_t>(), h->V.as<float>(), g.n_own, L, h->stream));
    if (is_bf16(h)) HIPCHK(h, launch_tile_f32_to_bf16(h->V.as<float>(), h->bV.as<uint16_t>(), h->ntiles_n, h->stream));
    return import_edges(h, 0, e);
} MGN_CATCH(h)

// Writes the owned rows into the caller's GLOBAL-shaped arrays (other rows are left untouched).
int mgn_latents_export(mgn_handle* h, float* v, float* e) try {
    if (int rc = need(h, false, true)) return rc;
    const LocalGraph& g = h->g;
    const int L = h->cfg.L;
    if (v) {
        if (is_bf16(h)) HIPCHK(h, launch_tile_bf16_to_f32(h->bV.as<uint16_t>(), h->V.as<float>(), h->ntiles_n, h->stream));
        const size_t vb = (size_t)g.N * L * 4;
        HIPCHK(h, h->stage.ensure(vb));
        if (h->cfg.nranks != 1) HIPCHK(h, hipMemcpyAsync(h->stage.p, v, vb, hipMemcpyHostToDevice, h->stream));   // keep foreign rows
        HIPCHK(h, launch_tiles_to_rows(h->V.as<float>(), nullptr, h->d_own_gid.as<int32_t>(), h->stage.as<float>(), g.n_own, L, h->stream));
        HIPCHK(h, hipMemcpyAsync(v, h->stage.p, vb, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    return export_edges(h, 0, e);
} MGN_CATCH(h)

int mgn_edge_latents_import(mgn_handle* h, int32_t set, const float* e) try {
    if (int rc = need(h, false, true)) return rc;
    if (set < 0 || set >= h->nsets) return fail(h, MGN_E_ARG, "mgn_edge_latents_import: set %d out of range", set);
    return import_edges(h, set, e);
} MGN_CATCH(h)

int mgn_edge_latents_export(mgn_handle* h, int32_t set, float* e) try {
    if (int rc = need(h, false, true)) return rc;
    if (set < 0 || set >= h->nsets) return fail(h, MGN_E_ARG, "mgn_edge_latents_export: set %d out of range", set);
    return export_edges(h, set, e);
} MGN_CATCH(h)

int mgn_latents_randn(mgn_handle* h, uint64_t seed) try {
    if (int rc = need(h, false, true)) return rc;
    const LocalGraph& g = h->g;
    HIPCHK(h, launch_randn_rows(h->V.as<float>(), nullptr, h->d_own_gid.as<int32_t>(), g.n_own, h->cfg.L, seed, h->stream));
    for (int q = 0; q < h->nsets; ++q)
        HIPCHK(h, launch_randn_rows(h->es[q].Elat.as<float>(), h->es[q].d_edge_gid.as<int64_t>(), nullptr, g.set[q].e_local, h->cfg.L,
                                    seed ^ (0xE5E5E5E5E5E5E5E5ull + (uint64_t)q * 0x9E3779B97F4A7C15ull), h->stream));
    if (is_bf16(h)) {
        HIPCHK(h, launch_tile_f32_to_bf16(h->V.as<float>(), h->bV.as<uint16_t>(), h->ntiles_n, h->stream));
        for (int q = 0; q < h->nsets; ++q)
            HIPCHK(h, launch_tile_f32_to_bf16(h->es[q].Elat.as<float>(), h->es[q].bElat.as<uint16_t>(), h->es[q].ntiles_e, h->stream));
    }
    return MGN_OK;
} MGN_CATCH(h)

// (sum, sum of squares) of the node latents and of the edge latents (all sets)
int mgn_latents_checksum(mgn_handle* h, double* sv, double* se, double* qv, double* qe) try {
    if (int rc = need(h, false, true)) return rc;
    const int np_ = checksum_partials();
    const int nb = 1 + h->nsets;
    if (is_bf16(h)) {
        HIPCHK(h, launch_tile_bf16_to_f32(h->bV.as<uint16_t>(), h->V.as<float>(), h->ntiles_n, h->stream));
        for (int q = 0; q < h->nsets; ++q)
            HIPCHK(h, launch_tile_bf16_to_f32(h->es[q].bElat.as<uint16_t>(), h->es[q].Elat.as<float>(), h->es[q].ntiles_e, h->stream));
    }
    HIPCHK(h, h->d_sum.ensure((size_t)nb * np_ * sizeof(double)));
    HIPCHK(h, launch_checksum(h->V.as<float>(), (int64_t)tile_floats(h->ntiles_n, h->cfg.L), h->d_sum.as<double>(), h->stream));
    for (int q = 0; q < h->nsets; ++q)
        HIPCHK(h, launch_checksum(h->es[q].Elat.as<float>(), (int64_t)tile_floats(h->es[q].ntiles_e, h->cfg.L),
                                  h->d_sum.as<double>() + (size_t)(1 + q) * np_, h->stream));
    std::vector<double> r((size_t)nb * np_);
    HIPCHK(h, hipMemcpyAsync(r.data(), h->d_sum.p, r.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    double acc[4] = {0, 0, 0, 0};   // bitwise reproducible: fixed partials, fixed order
    for (int b = 0; b < np_ / 2; ++b) {
        acc[0] += r[2 * b];
        acc[1] += r[2 * b + 1];
    }
    for (int q = 0; q < h->nsets; ++q)
        for (int b = 0; b < np_ / 2; ++b) {
            acc[2] += r[(size_t)(1 + q) * np_ + 2 * b];
            acc[3] += r[(size_t)(1 + q) * np_ + 2 * b + 1];
        }
    if (sv) *sv = acc[0];
    if (qv) *qv = acc[1];
    if (se) *se = acc[2];
    if (qe) *qe = acc[3];
    return MGN_OK;
} MGN_CATCH(h)


// ---- communicator and the staged multi-partition schedule -------------------------------------------
#define COMMCHK(h, expr)                                                                                   \
    do {                                                                                                   \
        if ((expr) != 0) return fail(h, MGN_E_RCCL, "%s: %s", #expr, (h)->comm ? (h)->comm->err.c_str() : "no communicator"); \
    } while (0)

extern "C++" int mgn::need_comm(mgn_handle* h, const char* who) {
    if (!h->comm) return fail(h, MGN_E_RCCL, "%s with nranks = %d needs a communicator: call mgn_comm_init on every rank first", who, h->cfg.nranks);
    return MGN_OK;
}

// per-peer byte layout of one exchange; rebuilt after every mgn_set_graph / mgn_set_edge_set
static int halo_plan(mgn_handle* h) {
    if (h->hx_ready) return MGN_OK;
    const LocalGraph& g = h->g;
    const int P = h->cfg.nranks;
    const size_t rowb = (size_t)mgn_halo_bytes_per_row(h);
    h->hx_sb.assign(P, 0); h->hx_so.assign(P, 0); h->hx_rb.assign(P, 0); h->hx_ro.assign(P, 0);
    size_t so = 0, ro = 0;
    for (int q = 0; q < P; ++q) {
        h->hx_sb[q] = (size_t)g.send_rows[q] * rowb; h->hx_so[q] = so; so += h->hx_sb[q];
        h->hx_rb[q] = (size_t)g.recv_rows[q] * rowb; h->hx_ro[q] = ro; ro += h->hx_rb[q];
    }
    // one edge set: the halo rows of P are one contiguous block in owner-rank order -- the layout of the receive buffer --
    // so the rows land there directly and no unpack copy runs
    h->hx_direct = h->nsets == 1 && !prows_blocked();   // (P rows are not contiguous: blocks of eight)
    if (!h->host_only) {
        HIPCHK(h, h->halo_send.ensure(so ? so : 16));
        if (!h->hx_direct) HIPCHK(h, h->halo_recv.ensure(ro ? ro : 16));
    }
    h->hx_ready = true;
    return MGN_OK;
}

static int exchange_start(mgn_handle* h) {
    if (int rc = halo_plan(h)) return rc;
    if (int rc = mgn_halo_pack(h, h->halo_send.p)) return rc;
    void* recv = h->halo_recv.p;
    if (h->hx_direct) {
        const size_t b = is_bf16(h) ? 2 : 4;
        recv = reinterpret_cast<char*>(is_bf16(h) ? h->es[0].bP.p : h->es[0].P.p) + (size_t)h->g.n_own * h->cfg.L * b;
    }
    COMMCHK(h, h->comm->a2a_start(h->halo_send.p, h->hx_sb.data(), h->hx_so.data(), recv, h->hx_rb.data(), h->hx_ro.data(), h->stream));
    return MGN_OK;
}

static int exchange_finish(mgn_handle* h) {
    COMMCHK(h, h->comm->a2a_finish(h->stream));
    if (!h->hx_direct) return mgn_halo_unpack(h, h->halo_recv.p);
    return MGN_OK;
}

// The schedule of one pass (the tested Python twin is engine.run_processor_staged): owned nodes are numbered boundary-first,
// so the boundary tiles are projected first, their P rows leave, and the interior projection plus the interior edge tiles of
// the next step run while the rows are on the wire; only the few boundary edge tiles wait for them.
static int project_and_start(mgn_handle* h, int k) {      // k = -1: projection for step 0
    if (int rc = mgn_proc_node_phase(h, k, 1)) return rc;
    if (int rc = exchange_start(h)) return rc;
    return mgn_proc_node_phase(h, k, 2);
}

static int processor_pass_staged(mgn_handle* h, int32_t nsteps, bool begin) {
    if (begin) {
        if (int rc = project_and_start(h, -1)) return rc;
    } else if (int rc = exchange_start(h)) return rc;      // P, Q of step 0 came from the encoder
    for (int k = 0; k < nsteps; ++k) {
        if (int rc = proc_edge_range(h, k, 1)) return rc;
        if (int rc = exchange_finish(h)) return rc;
        if (int rc = proc_edge_range(h, k, 2)) return rc;
        if (k + 1 < nsteps) {
            if (int rc = project_and_start(h, k)) return rc;
        } else if (int rc = mgn_proc_node(h, k, 0)) return rc;
    }
    return MGN_OK;
}

// every rank's (n_own, own_gid...) once per graph: output rows are gathered over the communicator
static int gather_plan(mgn_handle* h) {
    if (!h->all_gid.empty()) return MGN_OK;
    const LocalGraph& g = h->g;
    const int P = h->cfg.nranks;
    double mx = (double)g.n_own;
    COMMCHK(h, h->comm->allreduce_f64(&mx, 1, 1, h->stream));
    h->max_own = (int32_t)mx;
    const size_t per = (size_t)1 + h->max_own;
    std::vector<int32_t> mine(per, 0);
    mine[0] = g.n_own;
    memcpy(mine.data() + 1, g.own_gid.data(), (size_t)g.n_own * 4);
    HIPCHK(h, h->gath_s.ensure(per * 4));
    HIPCHK(h, h->gath_r.ensure(per * 4 * P));
    HIPCHK(h, hipMemcpyAsync(h->gath_s.p, mine.data(), per * 4, hipMemcpyHostToDevice, h->stream));
    COMMCHK(h, h->comm->allgather(h->gath_s.p, per * 4, h->gath_r.p, h->stream));
    std::vector<int32_t> all(per * P);
    HIPCHK(h, hipMemcpyAsync(all.data(), h->gath_r.p, per * 4 * P, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->all_gid.swap(all);
    return MGN_OK;
}

// local_dev [n_own][W] of every rank -> out [N][W] on the host, complete on every rank
extern "C++" int mgn::gather_rows_global(mgn_handle* h, const float* local_dev, int W, float* out) {
    if (int rc = gather_plan(h)) return rc;
    const LocalGraph& g = h->g;
    const int P = h->cfg.nranks;
    const size_t per = (size_t)h->max_own * W * 4;
    HIPCHK(h, h->gath_s.ensure(per ? per : 16));
    HIPCHK(h, h->gath_r.ensure(per ? per * P : 16));
    HIPCHK(h, hipMemcpyAsync(h->gath_s.p, local_dev, (size_t)g.n_own * W * 4, hipMemcpyDeviceToDevice, h->stream));
    COMMCHK(h, h->comm->allgather(h->gath_s.p, per, h->gath_r.p, h->stream));
    std::vector<float> all((size_t)h->max_own * W * P);
    HIPCHK(h, hipMemcpyAsync(all.data(), h->gath_r.p, per * P, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const size_t gper = (size_t)1 + h->max_own;
    for (int q = 0; q < P; ++q) {
        const int32_t* gq = h->all_gid.data() + (size_t)q * gper;
        const float* rows = all.data() + (size_t)q * h->max_own * W;
        for (int32_t i = 0; i < gq[0]; ++i) memcpy(out + (size_t)gq[1 + i] * W, rows + (size_t)i * W, (size_t)W * 4);
    }
    return MGN_OK;
}

// The once-per-call fold of a partitioned solve's sums (mgn_group_solver_grad*, mgn_group_rollout_eval): this rank's head [nhead] doubles
// (host) and acc [n] doubles (device; null: zeros) are gathered from every rank and added in ascending rank order, in double, by
// k_rank_sum_f64 on every rank -- head comes back as the ranks' sums, out [n] (device) as their sum rounded to fp32 once.  The same bits
// on every rank; blocks.  An allgather and one kernel, not allreduce_f64: the RCCL transport's allreduce does not promise an order.
extern "C++" int mgn::rank_fold_f64(mgn_handle* h, double* head, int64_t nhead, const double* acc, int64_t n, float* out) {
    const int P = h->cfg.nranks;
    const size_t stride = (size_t)rank_sum_f64_stride(nhead, n);
    HIPCHK(h, h->fold_s.ensure(stride * 8));
    HIPCHK(h, h->fold_r.ensure((stride * P + (size_t)nhead) * 8));
    double* s = h->fold_s.as<double>();
    double* r = h->fold_r.as<double>();
    HIPCHK(h, hipMemsetAsync(s, 0, stride * 8, h->stream));
    if (nhead > 0) HIPCHK(h, hipMemcpyAsync(s, head, (size_t)nhead * 8, hipMemcpyHostToDevice, h->stream));
    if (acc && n > 0) HIPCHK(h, hipMemcpyAsync(s + nhead, acc, (size_t)n * 8, hipMemcpyDeviceToDevice, h->stream));
    COMMCHK(h, h->comm->allgather(s, stride * 8, r, h->stream));
    HIPCHK(h, launch_rank_sum_f64(r, P, nhead, n, r + stride * P, out, h->stream));
    if (nhead > 0) HIPCHK(h, hipMemcpyAsync(head, r + stride * P, (size_t)nhead * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return MGN_OK;
}

// mgn.model(graph, ps, st) on a partitioned mesh: every rank encodes what it owns, the processor runs the staged schedule,
// the decoded rows are gathered so that every rank returns the complete output
static int forward_partitioned(mgn_handle* h, const float* nf, const float* ef, float* out) {
    if (int rc = need_comm(h, "mgn_forward")) return rc;
    if (int rc = need_set_features(h)) return rc;
    if (int rc = mgn_fwd_upload(h, nf, ef)) return rc;
    if (int rc = encode_impl(h, false)) return rc;
    if (int rc = processor_pass_staged(h, h->cfg.mps, false)) return rc;
    if (int rc = decode_impl(h, false)) return rc;
    return gather_rows_global(h, h->d_out.as<float>(), h->cfg.O, out);
}

static int processor_pass(mgn_handle* h, int32_t nsteps) {
    if (int rc = mgn_proc_begin(h)) return rc;
    return run_processor(h, nsteps);
}

// mgn_processor_steps_dev under ln_dims = MGN_LN_ALL (round 6): the resident latents leave their tiles as caller-order rows, the unfused
// whole-array driver (mgn_train.cpp: lnall_processor_steps; it takes device pointers) advances them, they go back.  Two row <-> tile passes
// per call on top of what mgn_processor_steps costs in this mode -- and no host copy.
static int lnall_processor_steps_dev(mgn_handle* h, int32_t nsteps) {
    if (int rc = need(h, true, true, true, true)) return rc;
    if (nsteps < 0 || nsteps > h->cfg.mps) return fail(h, MGN_E_ARG, "nsteps must be in [0, mps]");
    if (nsteps == 0) return MGN_OK;
    const LocalGraph& g = h->g;
    const EdgeTopo& t = g.set[0];
    auto& es = h->es[0];
    const int L = h->cfg.L;
    HIPCHK(h, h->lnall_v.ensure((size_t)(g.N > 0 ? g.N : 1) * L * 4));
    HIPCHK(h, h->lnall_e.ensure((size_t)(t.E > 0 ? t.E : 1) * L * 4));
    HIPCHK(h, launch_tiles_to_rows(h->V.as<float>(), nullptr, h->d_own_gid.as<int32_t>(), h->lnall_v.as<float>(), g.n_own, L, h->stream));
    if (t.e_local > 0)
        HIPCHK(h, launch_tiles_to_rows(es.Elat.as<float>(), es.d_edge_gid.as<int64_t>(), nullptr, h->lnall_e.as<float>(), t.e_local, L, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (int rc = lnall_processor_steps(h, h->lnall_v.as<float>(), h->lnall_e.as<float>(), nsteps)) return rc;   // (synchronises its stream)
    HIPCHK(h, launch_rows_to_tiles(h->lnall_v.as<float>(), nullptr, h->d_own_gid.as<int32_t>(), h->V.as<float>(), g.n_own, L, h->stream));
    if (t.e_local > 0)
        HIPCHK(h, launch_rows_to_tiles(h->lnall_e.as<float>(), es.d_edge_gid.as<int64_t>(), nullptr, es.Elat.as<float>(), t.e_local, L, h->stream));
    return MGN_OK;
}

int mgn_processor_steps_dev(mgn_handle* h, int32_t nsteps) try {
    if (h && !h->host_only && h->cfg.ln_dims == MGN_LN_ALL) return lnall_processor_steps_dev(h, nsteps);
    if (int rc = need(h, true, true)) return rc;
    if (nsteps < 0 || nsteps > h->cfg.mps) return fail(h, MGN_E_ARG, "nsteps must be in [0, mps]");
    if (nsteps == 0) return MGN_OK;
    if (h->cfg.nranks != 1 || (h->comm && h->force_staged)) {
        if (int rc = need_comm(h, "mgn_processor_steps_dev")) return rc;
        return processor_pass_staged(h, nsteps, true);
    }
    // Graph replay only helps launch-bound (small) passes; it needs a capturable stream (not the null stream) and no
    // per-launch event records.
#ifndef MGN_GRAPH_MAX_TILES
#define MGN_GRAPH_MAX_TILES 16384
#endif
    const bool graphable = h->use_graph && !h->prof && h->stream != nullptr && h->es[0].ntiles_e <= MGN_GRAPH_MAX_TILES;
    if (!graphable) return processor_pass(h, nsteps);
    if (h->graph_exec && h->graph_nsteps == nsteps) {
        HIPCHK(h, hipGraphLaunch(h->graph_exec, h->stream));
        return MGN_OK;
    }
    if (h->graph_warm != nsteps) {   // eager first: sets the per-kernel LDS attributes outside of any capture
        h->graph_warm = nsteps;
        return processor_pass(h, nsteps);
    }
    if (h->graph_exec) (void)hipGraphExecDestroy(h->graph_exec);
    h->graph_nsteps = -1;
    const int rc = capture_and_launch(h, h->stream, h->graph_exec, [&]() -> int { return processor_pass(h, nsteps); });
    if (h->graph_exec) h->graph_nsteps = nsteps;
    return rc;
} MGN_CATCH(h)

int mgn_processor_steps(mgn_handle* h, float* v, float* e, int32_t nsteps) try {
    if (h && !h->host_only && h->cfg.ln_dims == MGN_LN_ALL) return lnall_processor_steps(h, v, e, nsteps);
    if (int rc = need(h, true, true)) return rc;
    if (h->cfg.nranks != 1) return fail(h, MGN_E_STATE, "mgn_processor_steps drives one partition");
    if (int rc = mgn_latents_import(h, v, e)) return rc;
    if (int rc = mgn_processor_steps_dev(h, nsteps)) return rc;
    return mgn_latents_export(h, v, e);
} MGN_CATCH(h)

// ---- halo ------------------------------------------------------------------------------------------
// one halo row carries the P row of every edge set: [set 0: L][set 1: L]
int mgn_halo_bytes_per_row(const mgn_handle* h) { return h ? h->nsets * h->cfg.L * (h->cfg.dtype == MGN_BF16 ? 2 : 4) : MGN_E_ARG; }

int mgn_halo_pack(mgn_handle* h, void* send_dev) try {
    if (int rc = need(h, false, true)) return rc;
    const int64_t rows = (int64_t)h->g.send_idx.size();
    if (rows == 0) return MGN_OK;
    if (!send_dev) return fail(h, MGN_E_ARG, "mgn_halo_pack: null buffer");
    ProfScope ps(h, F_HALO);
    const int L = h->cfg.L, stride = h->nsets * L;
    for (int q = 0; q < h->nsets; ++q) {
        if (is_bf16(h))
            HIPCHK(h, launch_gather_rows16(h->es[q].bP.as<uint16_t>(), h->d_send_idx.as<int32_t>(),
                                           reinterpret_cast<uint16_t*>(send_dev) + (size_t)q * L, rows, stride, h->stream));
        else
            HIPCHK(h, launch_gather_rows(h->es[q].P.as<float>(), h->d_send_idx.as<int32_t>(), reinterpret_cast<float*>(send_dev) + (size_t)q * L,
                                         rows, L, stride, h->stream));
    }
    return MGN_OK;
} MGN_CATCH(nullptr)

int mgn_halo_unpack(mgn_handle* h, const void* recv_dev) try {
    if (int rc = need(h, false, true)) return rc;
    const LocalGraph& g = h->g;
    if (g.n_halo == 0) return MGN_OK;
    if (!recv_dev) return fail(h, MGN_E_ARG, "mgn_halo_unpack: null buffer");
    ProfScope ps(h, F_HALO);
    const size_t b = is_bf16(h) ? 2 : 4, rowb = (size_t)h->cfg.L * b;
    for (int q = 0; q < h->nsets; ++q) {
        if (is_bf16(h) && prows_blocked()) {
            HIPCHK(h, launch_scatter_prows16(reinterpret_cast<const uint16_t*>(recv_dev) + (size_t)q * h->cfg.L, h->nsets * h->cfg.L,
                                             h->es[q].bP.as<uint16_t>(), g.n_own, g.n_halo, h->stream));
            continue;
        }
        if (!is_bf16(h) && prows_blocked()) {
            HIPCHK(h, launch_scatter_prows(reinterpret_cast<const float*>(recv_dev) + (size_t)q * h->cfg.L, h->nsets * h->cfg.L, h->es[q].P.as<float>(),
                                           g.n_own, g.n_halo, h->cfg.L, h->stream));
            continue;
        }
        char* dst = reinterpret_cast<char*>(is_bf16(h) ? h->es[q].bP.p : h->es[q].P.p) + (size_t)g.n_own * rowb;
        HIPCHK(h, hipMemcpy2DAsync(dst, rowb, reinterpret_cast<const char*>(recv_dev) + (size_t)q * rowb, (size_t)h->nsets * rowb, rowb,
                                   (size_t)g.n_halo, hipMemcpyDeviceToDevice, h->stream));
    }
    return MGN_OK;
} MGN_CATCH(h)



// ---- device-side graph prologue (reference create_base_graph, src/graph.jl:25-55) ----------------------------
int mgn_triangles_to_edges_dev(mgn_handle* h, const int32_t* cells, int64_t n_cells, int32_t* senders, int32_t* receivers, int64_t capacity,
                               int64_t* n_directed) try {
    if (int rc = need(h, false, false)) return rc;
    if (!cells || n_cells < 0 || !n_directed || capacity < 0 || (capacity > 0 && (!senders || !receivers)))
        return fail(h, MGN_E_ARG, "mgn_triangles_to_edges_dev: bad argument");
    *n_directed = 0;
    if (n_cells == 0) return MGN_OK;
    const size_t cb = (size_t)n_cells * 3 * 4;
    HIPCHK(h, h->gpos.ensure(cb));
    HIPCHK(h, hipMemcpyAsync(h->gpos.p, cells, cb, hipMemcpyDefault, h->stream));      // host or device source
    HIPCHK(h, h->gout.ensure((size_t)(capacity > 0 ? capacity : 1) * 8));
    int32_t* ds = h->gout.as<int32_t>();
    int32_t* dr = ds + (capacity > 0 ? capacity : 1);
    int64_t m = 0;
    const hipError_t e = dev_triangles_to_edges(h->gpos.as<int32_t>(), n_cells, h->gwork, ds, dr, capacity, &m, h->stream);
    *n_directed = 2 * m;
    if (e == hipErrorInvalidValue && 2 * m > capacity)
        return fail(h, MGN_E_ARG, "mgn_triangles_to_edges_dev: %lld directed edges do not fit the buffers (capacity %lld; 6 x n_cells always does)",
                    (long long)(2 * m), (long long)capacity);
    HIPCHK(h, e);
    HIPCHK(h, hipMemcpyAsync(senders, ds, (size_t)(2 * m) * 4, hipMemcpyDefault, h->stream));
    HIPCHK(h, hipMemcpyAsync(receivers, dr, (size_t)(2 * m) * 4, hipMemcpyDefault, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return MGN_OK;
} MGN_CATCH(h)

int mgn_set_static_mesh(mgn_handle* h, const int32_t* node_type, int32_t type_min, int32_t type_max, const float* mesh_pos, int32_t pos_dim,
                        const float* val_mask) try {
    if (int rc = need(h, true, true)) return rc;
    const mgn_config& c = h->cfg;
    if (c.nranks != 1) return fail(h, MGN_E_STATE, "mgn_set_static_mesh drives one partition");
    if (h->nsets != 1) return fail(h, MGN_E_STATE, "mgn_set_static_mesh mirrors the reference's single-edge-set create_base_graph (src/graph.jl:25-55)");
    if (!node_type || !mesh_pos || type_max < type_min) return fail(h, MGN_E_ARG, "mgn_set_static_mesh: bad argument");
    const int depth = type_max - type_min + 1;
    if (c.Fn - c.O != depth) return fail(h, MGN_E_ARG, "mgn_set_static_mesh: Fn - O = %d but the one-hot depth is %d", c.Fn - c.O, depth);
    if (c.Fe != pos_dim + 1) return fail(h, MGN_E_ARG, "mgn_set_static_mesh: Fe = %d but mesh_pos has %d columns (Fe = dims + 1, src/graph.jl:49-52)", c.Fe, pos_dim);
    const LocalGraph& g = h->g;
    invalidate_static(h);
    h->in_wa = c.O;
    h->in_wb = depth;
    h->in_local = true;          // the static inputs are produced in ENGINE order (owned nodes, receiver-sorted local edges)
    HIPCHK(h, h->d_nfA.ensure((size_t)g.N * c.O * 4));
    HIPCHK(h, h->d_nfB.ensure((size_t)g.n_own * depth * 4));
    HIPCHK(h, h->es[0].d_ef.ensure((size_t)(g.set[0].e_local > 0 ? g.set[0].e_local : 1) * c.Fe * 4));
    HIPCHK(h, h->gtype.ensure((size_t)g.N * 4));
    HIPCHK(h, h->gpos.ensure((size_t)g.N * pos_dim * 4));
    HIPCHK(h, hipMemcpyAsync(h->gtype.p, node_type, (size_t)g.N * 4, hipMemcpyDefault, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->gpos.p, mesh_pos, (size_t)g.N * pos_dim * 4, hipMemcpyDefault, h->stream));
    // one partition: no boundary block; local ids are global ids unless mgn_set_graph renumbered the mesh (then through own_gid)
    const int32_t* l2g = g.renumbered ? h->d_own_gid.as<int32_t>() : nullptr;
    HIPCHK(h, launch_one_hot(h->gtype.as<int32_t>(), l2g, g.n_own, type_min, depth, h->d_nfB.as<float>(), h->stream));
    HIPCHK(h, launch_edge_features_local(h->gpos.as<float>(), pos_dim, h->es[0].d_snd.as<int32_t>(), h->es[0].d_rcv.as<int32_t>(), l2g,
                                         g.set[0].e_local, h->es[0].d_ef.as<float>(), h->stream));
    h->have_mask = val_mask != nullptr;
    if (val_mask) {
        HIPCHK(h, h->d_mask.ensure((size_t)g.N * 4));
        HIPCHK(h, hipMemcpyAsync(h->d_mask.p, val_mask, (size_t)g.N * 4, hipMemcpyDefault, h->stream));
    }
    if (int rc = encode_impl(h, true, false, true)) return rc;       // edge encoder: once per trajectory
    const bool bf = is_bf16(h);
    const size_t eb = tile_floats(h->es[0].ntiles_e, c.L) * (bf ? 2 : 4);
    HIPCHK(h, h->es[0].elat0.ensure(eb));
    HIPCHK(h, hipMemcpyAsync(h->es[0].elat0.p, bf ? h->es[0].bElat.p : h->es[0].Elat.p, eb, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->have_static = true;
    return MGN_OK;
} MGN_CATCH(h)

int mgn_world_edges_dev(mgn_handle* h, int32_t set, const float* world_pos, int32_t dim, float radius, int64_t* n_edges) try {
    if (int rc = need(h, false, true)) return rc;
    if (h->cfg.nranks != 1) return fail(h, MGN_E_STATE, "mgn_world_edges_dev drives one partition (with nranks > 1 search on the host: mgn_world_edges + mgn_set_edge_set)");
    if (set < 1 || set >= h->nsets) return fail(h, MGN_E_ARG, "mgn_world_edges_dev: set %d out of range (handle has %d edge sets)", set, h->nsets);
    if (!world_pos || dim < 1 || dim > 3 || !(radius > 0.f)) return fail(h, MGN_E_ARG, "mgn_world_edges_dev: bad argument");
    LocalGraph& g = h->g;
    auto& es = h->es[set];
    h->hx_ready = false;
    invalidate_static(h);
    train_invalidate(h, 2);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    drop_graph(h);
    HIPCHK(h, h->gpos.ensure((size_t)g.N * dim * 4));
    if (g.renumbered) {   // the search runs in the engine's node numbering (set 0's adjacency is held in it): positions gathered through own_gid
        HIPCHK(h, h->stage.ensure((size_t)g.N * dim * 4));
        HIPCHK(h, hipMemcpyAsync(h->stage.p, world_pos, (size_t)g.N * dim * 4, hipMemcpyDefault, h->stream));
        HIPCHK(h, launch_permute_rows(h->gpos.as<float>(), h->stage.as<float>(), h->d_own_gid.as<int32_t>(), g.N, dim, false, h->stream));
    } else {
        HIPCHK(h, hipMemcpyAsync(h->gpos.p, world_pos, (size_t)g.N * dim * 4, hipMemcpyDefault, h->stream));
    }
    int64_t E = 0;
    const hipError_t e = dev_world_edges(h->gpos.as<float>(), dim, g.N, radius, h->es[0].d_rowptr.as<int32_t>(), h->es[0].d_snd.as<int32_t>(), h->gwork,
                                         es.d_snd, es.d_rcv, es.d_rowptr, &E, h->stream);
    if (e == hipErrorInvalidValue) return fail(h, MGN_E_ARG, "mgn_world_edges_dev: non-finite position");
    HIPCHK(h, e);
    // the set lives on the device only (receiver-major == engine order, global edge id == position): no host lists are kept
    EdgeTopo& t = g.set[set];
    t.E = t.e_local = E;
    t.halo_span = 0;
    t.snd.clear(); t.rcv.clear(); t.rowptr.clear(); t.edge_gid.clear();
    es.gs.clear(); es.gr.clear();
    es.ntiles_e = (int32_t)((E + TILE - 1) / TILE);
    HIPCHK(h, es.d_edge_gid.ensure((size_t)(E > 0 ? E : 1) * 8));
    HIPCHK(h, launch_iota64(es.d_edge_gid.as<int64_t>(), E, h->stream));
    if (int rc = alloc_edge_set(h, set)) return rc;
    es.have_ef = false;
    if (es.Fe == dim + 1) {      // [rel world pos ; norm]: the world-edge features of the cloth models, straight into the encoder's input
        HIPCHK(h, es.d_ef.ensure((size_t)(E > 0 ? E : 1) * es.Fe * 4));
        HIPCHK(h, launch_edge_features_local(h->gpos.as<float>(), dim, es.d_snd.as<int32_t>(), es.d_rcv.as<int32_t>(), nullptr, E, es.d_ef.as<float>(), h->stream));
        es.have_ef = true;
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (n_edges) *n_edges = E;
    return MGN_OK;
} MGN_CATCH(h)

/* the device-built set's topology, for hosts that want it (tests): senders / receivers [E] 0-based, receiver-major */
int mgn_edge_set_export(mgn_handle* h, int32_t set, int32_t* senders, int32_t* receivers) try {
    if (int rc = need(h, false, true)) return rc;
    if (set < 0 || set >= h->nsets) return fail(h, MGN_E_ARG, "mgn_edge_set_export: set %d out of range", set);
    if (h->cfg.nranks != 1) return fail(h, MGN_E_STATE, "mgn_edge_set_export drives one partition");
    const int64_t E = h->g.set[set].e_local;
    if (E > 0 && (!senders || !receivers)) return fail(h, MGN_E_ARG, "mgn_edge_set_export: null output");
    // every array crosses the boundary in the CALLER's node numbering: a renumbered handle (graph_host.h) holds engine-order ids and maps
    // them back on the host -- so it is decided BEFORE anything is written whether the outputs can be walked by the host (a device
    // output on a renumbered handle is refused with its buffers untouched; an output the runtime cannot classify counts as device memory
    // unless it is plain host memory the runtime has never seen)
    if (h->g.renumbered && E > 0) {
        for (const int32_t* p : {senders, receivers}) {
            hipPointerAttribute_t at{};
            const hipError_t e = hipPointerGetAttributes(&at, p);
            (void)hipGetLastError();
            const bool host_walkable = e == hipErrorInvalidValue /* unregistered host memory */ ||
                                       (e == hipSuccess && (at.type == hipMemoryTypeHost || at.type == hipMemoryTypeUnregistered || at.type == hipMemoryTypeManaged));
            if (!host_walkable) return fail(h, MGN_E_UNSUPPORTED, "mgn_edge_set_export: device output on a renumbered handle (pass host arrays)");
        }
    }
    if (E > 0) {
        HIPCHK(h, hipMemcpyAsync(senders, h->es[set].d_snd.p, (size_t)E * 4, hipMemcpyDefault, h->stream));
        HIPCHK(h, hipMemcpyAsync(receivers, h->es[set].d_rcv.p, (size_t)E * 4, hipMemcpyDefault, h->stream));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (h->g.renumbered && E > 0) {
        for (int64_t j = 0; j < E; ++j) {
            senders[j] = h->g.own_gid[(size_t)senders[j]];
            receivers[j] = h->g.own_gid[(size_t)receivers[j]];
        }
    }
    return MGN_OK;
} MGN_CATCH(h)

// ---- communicator entry points ---------------------------------------------------------------------------------------
int mgn_comm_unique_id(void* id, int32_t transport) try {
    if (!id) return fail(nullptr, MGN_E_ARG, "mgn_comm_unique_id: null id");
    std::string why;
    if (comm_unique_id(id, transport, why) != 0) return fail(nullptr, MGN_E_RCCL, "mgn_comm_unique_id: %s", why.c_str());
    return MGN_OK;
} MGN_CATCH(nullptr)

int mgn_comm_init(mgn_handle* h, const void* id, size_t id_bytes, int32_t transport) try {
    if (!h) return MGN_E_ARG;
    if (!id || id_bytes != MGN_COMM_ID_BYTES) return fail(h, MGN_E_ARG, "mgn_comm_init: id must be MGN_COMM_ID_BYTES (%d) bytes", MGN_COMM_ID_BYTES);
    if (transport != MGN_COMM_RCCL && transport != MGN_COMM_HOST && transport != MGN_COMM_LOCAL)
        return fail(h, MGN_E_ARG, "mgn_comm_init: unknown transport %d", transport);
    if (h->comm) return fail(h, MGN_E_STATE, "mgn_comm_init: the handle already has a communicator (mgn_comm_destroy first)");
    if (!h->host_only) HIPCHK(h, hipStreamSynchronize(h->stream));
    std::string why;
    h->comm = comm_create(id, transport, h->cfg.rank, h->cfg.nranks, !h->host_only, why);
    if (!h->comm) return fail(h, MGN_E_RCCL, "mgn_comm_init: %s", why.c_str());
    h->force_staged = env_int("MGN_FORCE_STAGED", h->force_staged);
    h->hx_ready = false;
    h->all_gid.clear();
    if (!h->host_only) drop_graph(h);
    return MGN_OK;
} MGN_CATCH(h)

// File bootstrap of the communicator id (single node, no launcher store).  A file left behind by an earlier run (or a crash) must
// never be taken for this run's id, so the id travels with a nonce and is confirmed both ways:
//   rank 0: removes path, path.go and stale acks; writes path = {id, nonce}; waits until every other rank has written
//           path.ack.<rank> = nonce; writes path.go = nonce; after the collective mgn_comm_init has returned removes every file.
//   rank r: reads path, writes its ack with the nonce it read, waits for a path.go that carries the same nonce AND is not older
//           than its own ack (a stale go predates it); on a different nonce it starts over with a fresh read of path.
namespace {
struct IdFile { unsigned char id[MGN_COMM_ID_BYTES]; uint64_t nonce; };
bool write_atomic(const std::string& path, const void* data, size_t n) {
    const std::string tmp = path + ".tmp";
    FILE* f = fopen(tmp.c_str(), "wb");
    if (!f) return false;
    const bool ok = fwrite(data, 1, n, f) == n;
    fclose(f);
    return ok && rename(tmp.c_str(), path.c_str()) == 0;
}
bool read_exact(const std::string& path, void* data, size_t n) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return false;
    const size_t got = fread(data, 1, n, f);
    fclose(f);
    return got == n;
}
double mtime_of(const std::string& path) {
    struct stat st;
    if (stat(path.c_str(), &st) != 0) return -1.0;
    return (double)st.st_mtim.tv_sec + 1e-9 * (double)st.st_mtim.tv_nsec;
}
void nap20ms() {
    struct timespec ts = {0, 20 * 1000 * 1000};
    nanosleep(&ts, nullptr);
}
}  // namespace

int mgn_comm_init_file(mgn_handle* h, const char* path, int32_t transport) try {
    if (!h || !path) return fail(h, MGN_E_ARG, "mgn_comm_init_file: null argument");
    const double limit = env_double("MGN_COMM_TIMEOUT_S", 120.0);
    const std::string base(path), go = base + ".go";
    const int rank = h->cfg.rank, nranks = h->cfg.nranks;
    auto ack_of = [&](int r) { return base + ".ack." + std::to_string(r); };
    IdFile rec{};
    if (rank == 0) {
        unlink(path);
        unlink(go.c_str());
        for (int r = 1; r < nranks; ++r) unlink(ack_of(r).c_str());
        if (int rc = mgn_comm_unique_id(rec.id, transport)) return fail(h, rc, "%s", mgn_last_error(nullptr));
        struct timespec now;
        clock_gettime(CLOCK_REALTIME, &now);
        rec.nonce = ((uint64_t)now.tv_sec << 32) ^ ((uint64_t)now.tv_nsec << 8) ^ (uint64_t)getpid();
        FILE* ur = fopen("/dev/urandom", "rb");
        if (ur) { uint64_t x = 0; if (fread(&x, 1, 8, ur) == 8) rec.nonce ^= x; fclose(ur); }
        if (!write_atomic(base, &rec, sizeof rec)) return fail(h, MGN_E_RCCL, "mgn_comm_init_file: cannot write %s", path);
        double waited = 0;
        for (int r = 1; r < nranks; ++r)
            for (;;) {
                uint64_t n = 0;
                if (read_exact(ack_of(r), &n, 8) && n == rec.nonce) break;
                if (waited > limit) return fail(h, MGN_E_RCCL, "mgn_comm_init_file: timed out waiting for rank %d to acknowledge %s", r, path);
                nap20ms();
                waited += 0.02;
            }
        if (!write_atomic(go, &rec.nonce, 8)) return fail(h, MGN_E_RCCL, "mgn_comm_init_file: cannot write %s", go.c_str());
    } else {
        double waited = 0;
        for (bool confirmed = false; !confirmed;) {
            while (!read_exact(base, &rec, sizeof rec)) {
                if (waited > limit) return fail(h, MGN_E_RCCL, "mgn_comm_init_file: timed out waiting for rank 0 to write %s", path);
                nap20ms();
                waited += 0.02;
            }
            if (!write_atomic(ack_of(rank), &rec.nonce, 8)) return fail(h, MGN_E_RCCL, "mgn_comm_init_file: cannot write %s", ack_of(rank).c_str());
            const double t_ack = mtime_of(ack_of(rank));
            for (;;) {
                uint64_t n = 0;
                if (read_exact(go, &n, 8) && mtime_of(go) >= t_ack) {
                    confirmed = n == rec.nonce;
                    break;                                   // a go for another nonce: what this rank read was stale -> read again
                }
                IdFile cur{};
                if (read_exact(base, &cur, sizeof cur) && cur.nonce != rec.nonce) break;   // rank 0 has published a new id meanwhile
                if (waited > limit) return fail(h, MGN_E_RCCL, "mgn_comm_init_file: timed out waiting for rank 0 to confirm %s", path);
                nap20ms();
                waited += 0.02;
            }
            if (!confirmed) { nap20ms(); waited += 0.02; }
        }
    }
    const int rc = mgn_comm_init(h, rec.id, MGN_COMM_ID_BYTES, transport);
    if (rank == 0) {                                         // the collective init is over on every rank that could reach it
        unlink(path);
        unlink(go.c_str());
        for (int r = 1; r < nranks; ++r) unlink(ack_of(r).c_str());
    }
    return rc;
} MGN_CATCH(h)

int mgn_comm_destroy(mgn_handle* h) try {
    if (!h) return MGN_E_ARG;
    if (!h->host_only) (void)hipStreamSynchronize(h->stream);
    delete h->comm;
    h->comm = nullptr;
    h->hx_ready = false;
    h->all_gid.clear();
    return MGN_OK;
} MGN_CATCH(h)

int mgn_comm_barrier(mgn_handle* h) try {
    if (!h) return MGN_E_ARG;
    if (int rc = need_comm(h, "mgn_comm_barrier")) return rc;
    COMMCHK(h, h->comm->barrier(h->stream));
    return MGN_OK;
} MGN_CATCH(h)

int mgn_comm_allreduce(mgn_handle* h, double* x, int32_t n, int32_t op) try {
    if (!h) return MGN_E_ARG;
    if (int rc = need_comm(h, "mgn_comm_allreduce")) return rc;
    if (!x || n < 0 || (op != 0 && op != 1)) return fail(h, MGN_E_ARG, "mgn_comm_allreduce: bad argument");
    COMMCHK(h, h->comm->allreduce_f64(x, n, op, h->stream));
    return MGN_OK;
} MGN_CATCH(h)

int mgn_halo_exchange(mgn_handle* h) try {
    if (int rc = need(h, false, true)) return rc;
    if (int rc = need_comm(h, "mgn_halo_exchange")) return rc;
    if (int rc = exchange_start(h)) return rc;
    return exchange_finish(h);
} MGN_CATCH(h)

int mgn_halo_exchange_host(mgn_handle* h, const float* own_rows, float* halo_rows, int32_t width) try {
    if (!h || !h->have_graph) return fail(h, MGN_E_STATE, "mgn_halo_exchange_host before mgn_set_graph");
    if (int rc = need_comm(h, "mgn_halo_exchange_host")) return rc;
    if (width < 1 || (!own_rows && h->g.n_own) || (!halo_rows && h->g.n_halo)) return fail(h, MGN_E_ARG, "mgn_halo_exchange_host: bad argument");
    const LocalGraph& g = h->g;
    const int P = h->cfg.nranks;
    const size_t rowb = (size_t)width * 4;
    std::vector<float> send(g.send_idx.size() * (size_t)width);
    for (size_t i = 0; i < g.send_idx.size(); ++i) memcpy(send.data() + i * width, own_rows + (size_t)g.send_idx[i] * width, rowb);
    std::vector<size_t> sb(P), so(P), rb(P), ro(P);
    size_t s0 = 0, r0 = 0;
    for (int q = 0; q < P; ++q) {
        sb[q] = (size_t)g.send_rows[q] * rowb; so[q] = s0; s0 += sb[q];
        rb[q] = (size_t)g.recv_rows[q] * rowb; ro[q] = r0; r0 += rb[q];
    }
    COMMCHK(h, h->comm->a2a_host(send.data(), sb.data(), so.data(), halo_rows, rb.data(), ro.data()));
    return MGN_OK;
} MGN_CATCH(h)

// tests (not part of the public header): one sparse all-to-all-v through the handle's communicator on the handle's stream, at sizes
// and alignments the engine never produces.  send_dev / recv_dev: device buffers; sbytes, soff, rbytes, roff: [nranks] as Comm::a2a_start
// takes them.  Enqueues only; mgn_synchronize before reading recv_dev.
int mgn_debug_comm_a2a(mgn_handle* h, const void* send_dev, const size_t* sbytes, const size_t* soff, void* recv_dev, const size_t* rbytes,
                       const size_t* roff) try {
    if (int rc = need(h, false, false)) return rc;
    if (int rc = need_comm(h, "mgn_debug_comm_a2a")) return rc;
    if (!sbytes || !soff || !rbytes || !roff) return fail(h, MGN_E_ARG, "mgn_debug_comm_a2a: null argument");
    COMMCHK(h, h->comm->a2a_start(send_dev, sbytes, soff, recv_dev, rbytes, roff, h->stream));
    COMMCHK(h, h->comm->a2a_finish(h->stream));
    return MGN_OK;
} MGN_CATCH(h)

// Process-wide kernel-path override for tests (not part of the public header): 0 auto, 1 LDS-resident persistent
// kernels, 2 all-streaming, 3 cooperative 4-wave tiles.  Returns the previous value.
int mgn_debug_kernel_path(int path) { return set_kernel_path(path); }
int mgn_debug_c16_row_tiles(int rt) { return set_c16_row_tiles(rt); }
int mgn_debug_c16_edge_tiles(int t) { return set_c16_edge_tiles(t); }   // size limit of the 16-row kernels in edge tiles per CU (0: by the handle)
// large fp32 launches: 1 split path (k_edge_ring + k_node_split + k_project_split: bf16 matrix cores at fp32 accuracy; the default),
// 0 fp32-MFMA kernels; returns the old value
int mgn_debug_fp32_split(int on) { return set_fp32_split(on); }
// 1 (default): the split path computes on two fp16 pieces per operand and three piece products (k_edge_ring_h), 0: on three bf16 pieces
// and six products (k_edge_ring); returns the old value
int mgn_debug_split_f16(int on) { return set_split_f16(on); }
// split path on two fp16 pieces: 1 (default) k_edge_ring_hs (every weight piece streamed, family codes 16 / 17), 0 k_edge_ring_h (13 / 14);
// MGN_RINGH_STREAM is the initial value; returns the old value
int mgn_debug_ringh_stream(int on) { return set_ringh_stream(on); }
// 1 (default): node MLP + projection of the next step as one k_node_ring_hs launch where both would run (family code 11), 0: k_node_split_h
// (10) + k_project_split_h; MGN_NODE_RING_HS is the initial value; returns the old value
int mgn_debug_node_ring_hs(int on) { return set_node_ring_hs(on); }
// tests: the CU count that every size decision of the inference launches reads, so that a small mesh reaches the kernels, block shapes and
// tile walks of a mesh (device CUs / n) times its size.  n = 0: the device's own count; otherwise a multiple of 8 (one block per XCD label)
// from 8 up to the device's count.  Returns the old value (0: none was set), -1 if n is refused (nothing changes).
int mgn_debug_num_cus(int n) { return set_num_cus(n); }
// the same switch for the streaming kernels of the training step (train.hip: train_chunk); returns the old value
int mgn_debug_train_f16(int on) { return set_train_f16(on); }
// tests: every chunk the device packed (k_pack_weights) against the host functions that specify the layouts; returns the number of
// elements that differ (0 = bitwise equal), < 0 on error
long long mgn_debug_pack_check(mgn_handle* h) try {
    if (int rc = need(h, true, false)) return -rc;
    const int L = h->cfg.L;
    const size_t CH = (size_t)L * L;
    const float* p = nullptr;
    if (int rc = host_params(h, &p)) return -rc;
    long long bad = 0;
    std::vector<float> hf(3 * CH), df(3 * CH);
    std::vector<uint16_t> hb(3 * 16384), db(3 * 16384);
    for (const WPackJob& jb : h->wjobs) {
        const float* W = p + jb.src;
        if (jb.kind == 0) {
            const size_t n = (L == 128 ? 3 : 2) * CH;
            pack_chunk(hf.data(), W, jb.ldw, jb.kbase, L);
            pack_chunk_tmajor(hf.data() + CH, hf.data(), L);
            if (L == 128) pack_chunk16(hf.data() + 2 * CH, W, jb.ldw, jb.kbase);
            if (hipMemcpy(df.data(), h->wfrag.as<float>() + jb.off, n * 4, hipMemcpyDeviceToHost) != hipSuccess) return -MGN_E_HIP;
            for (size_t i = 0; i < n; ++i) bad += memcmp(&hf[i], &df[i], 4) != 0;
        } else if (jb.kind == 3) {
            pack_chunk_bf16(hb.data(), W, jb.ldw, jb.kbase);
            if (hipMemcpy(db.data(), h->wbf.as<uint16_t>() + jb.off, 16384 * 2, hipMemcpyDeviceToHost) != hipSuccess) return -MGN_E_HIP;
            for (size_t i = 0; i < 16384; ++i) bad += hb[i] != db[i];
        } else if (jb.kind == 4 || jb.kind == 5) {
            pack_chunk_split_h(hb.data(), W, jb.ldw, jb.kbase, jb.scale, jb.kind == 5);
            if (hipMemcpy(db.data(), h->wsp.as<uint16_t>() + jb.off, 2 * 16384 * 2, hipMemcpyDeviceToHost) != hipSuccess) return -MGN_E_HIP;
            for (size_t i = 0; i < 2 * 16384; ++i) bad += hb[i] != db[i];
        } else {
            pack_chunk_split(hb.data(), W, jb.ldw, jb.kbase, jb.kind == 2);
            if (hipMemcpy(db.data(), h->wsp.as<uint16_t>() + jb.off, 3 * 16384 * 2, hipMemcpyDeviceToHost) != hipSuccess) return -MGN_E_HIP;
            for (size_t i = 0; i < 3 * 16384; ++i) bad += hb[i] != db[i];
        }
    }
    return bad;
} catch (...) { return -MGN_E_OOM; }
int mgn_debug_c16_split(int on) { return set_c16_split(on); }   // bits: 1 edge kernel (default), 2 node kernel, 4 edge kernel at one row tile per block; 0: fp32 MFMA pipe (kernels.hip)
int mgn_debug_last_node_kernel(void) { return last_node_kernel(); }   // the same for the node MLP (codes: kernels.hip, launch_node_step)
int mgn_debug_last_edge_kernel(void) { return last_edge_kernel(); }   // kernels.hip: which family the last fp32 edge launch ran on
// node numbering policy of the NEXT mgn_set_graph calls (0 never, 1 auto, 2 always breadth-first); returns the old value
int mgn_debug_renumber(int mode) { return g_renumber.set(mode); }
// tests: the row maximum the two-piece split kernels scale a row by (split_common.hpp: h2_rowmax<abs != 0>) and h2_scale's pair for it, of
// nrows >= 1 rows of 128 floats each (host arrays; amax, s, rs: [nrows]).  abs != 0: max |x|; abs == 0: max(x, 0)
int mgn_debug_rowmax(const float* rows, int nrows, int abs, float* amax, float* s, float* rs) {
    if (!rows || !amax || !s || !rs || nrows < 1) return MGN_E_ARG;
    return debug_rowmax(rows, nrows, abs, amax, s, rs) == hipSuccess ? MGN_OK : MGN_E_HIP;
}
int mgn_debug_renumbered(const mgn_handle* h) { return h && h->have_graph && h->g.renumbered ? 1 : 0; }

int mgn_debug_edge_stamps(mgn_handle* h, int32_t k, unsigned long long* out /* [32768] */) try {
    if (int rc = need(h, true, true)) return rc;
    const size_t n = 32768;
    HIPCHK(h, h->d_stamps.ensure(n * 8));
    HIPCHK(h, hipMemsetAsync(h->d_stamps.p, 0, n * 8, h->stream));
    if (int rc = mgn_proc_edge(h, k)) return rc;
    HIPCHK(h, hipMemcpyAsync(out, h->d_stamps.p, n * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->d_stamps.release();
    return MGN_OK;
} MGN_CATCH(h)

int mgn_debug_node_stamps(mgn_handle* h, int32_t k, unsigned long long* out /* [32768] */) try {
    if (int rc = need(h, true, true)) return rc;
    const size_t n = 32768;
    HIPCHK(h, h->d_stamps.ensure(n * 8));
    HIPCHK(h, hipMemsetAsync(h->d_stamps.p, 0, n * 8, h->stream));
    if (int rc = mgn_proc_node(h, k, 1)) return rc;
    HIPCHK(h, hipMemcpyAsync(out, h->d_stamps.p, n * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->d_stamps.release();
    return MGN_OK;
} MGN_CATCH(h)

// ---- profiling ---------------------------------------------------------------------------------------
int mgn_profile_enable(mgn_handle* h, int32_t on) try {
    if (int rc = need(h, false, false)) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (auto& r : h->recs) {
        h->event_pool.push_back(r.a);
        h->event_pool.push_back(r.b);
    }
    h->recs.clear();
    h->prof = on != 0;
    // events are created here, outside of whatever the caller is about to time (one per scope boundary; the pool grows on
    // demand beyond this)
    while (h->prof && h->event_pool.size() < 4096) {
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) break;
        h->event_pool.push_back(e);
    }
    return MGN_OK;
} MGN_CATCH(h)

int mgn_profile_read(mgn_handle* h, double ms_avg[8], int64_t counts[8]) try {
    if (!h || !ms_avg || !counts) return MGN_E_ARG;
    if (int rc = need(h, false, false)) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    double tot[8] = {0};
    int64_t cnt[8] = {0};
    for (auto& r : h->recs) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
            tot[r.fam] += ms;
            cnt[r.fam] += 1;
        }
        h->event_pool.push_back(r.a);
        h->event_pool.push_back(r.b);
    }
    h->recs.clear();
    for (int i = 0; i < 8; ++i) {
        ms_avg[i] = cnt[i] ? tot[i] / (double)cnt[i] : 0.0;
        counts[i] = cnt[i];
    }
    return MGN_OK;
} MGN_CATCH(h)

}  // extern "C"
