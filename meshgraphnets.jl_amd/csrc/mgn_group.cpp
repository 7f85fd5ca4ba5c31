// mgn_group: one handle that drives the P partitions of a mesh from one caller thread (include/mgn_hip.h, "one process, P partitions").
// Inside it is what the tests' thread-ranks are: one worker thread per rank, each owning an ordinary rank handle, joined by one
// MGN_COMM_LOCAL communicator (comm.cpp).  A group call is the same mgn_* call on every worker.
#include <atomic>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>
#include <mutex>
#include <thread>

#include "engine_internal.h"

#pragma GCC visibility push(hidden)   // (the members are not part of the library's dynamic symbols)
struct mgn_group {
    mgn_config cfg{};
    int P = 0;
    bool host_only = false;
    std::vector<int32_t> devices;
    std::vector<mgn_handle*> h;
    std::string err;
    unsigned char id[MGN_COMM_ID_BYTES] = {};
    bool have_comm = false;
    int32_t N = 0;                                   // of the last mgn_group_set_graph (sizes of the scratch outputs)

    // dispatch: `job` is run by every worker (or by `only` alone) for ticket `epoch`; the caller waits for `left` to reach 0
    std::vector<std::thread> workers;
    std::mutex mu;
    std::condition_variable cv_go, cv_done;
    uint64_t epoch = 0;
    int only = -1, left = 0;
    bool quit = false;
    std::function<int(int)> job;
    std::vector<int> rc;
    std::vector<int> order;                          // order[k]: rank k was the order[k]-th to fail in this call (0: it did not)
    std::atomic<int> nfailed{0};
    std::vector<std::vector<char>> scratch;          // [rank]: outputs of the ranks other than 0

    void work(int k) {
        if (devices[k] >= 0) (void)hipSetDevice(devices[k]);   // once: every call of this rank runs on this thread
        uint64_t seen = 0;
        for (;;) {
            std::unique_lock<std::mutex> lock(mu);
            cv_go.wait(lock, [&] { return quit || epoch != seen; });
            if (quit) return;
            seen = epoch;
            if (only >= 0 && only != k) continue;
            lock.unlock();
            int r;
            try {
                r = job(k);
            } catch (...) {
                r = MGN_E_OOM;
            }
            if (r != MGN_OK) {
                // the peers may be inside a collective that this rank will never join: they leave it now, not after the time limit
                order[k] = nfailed.fetch_add(1) + 1;
                if (have_comm) mgn::comm_local_abort(id);
            }
            lock.lock();
            rc[k] = r;
            if (--left == 0) cv_done.notify_all();
        }
    }
    void dispatch(std::function<int(int)> f, int one) {
        std::unique_lock<std::mutex> lock(mu);
        job = std::move(f);
        only = one;
        left = one >= 0 ? 1 : P;
        std::fill(rc.begin(), rc.end(), MGN_OK);
        std::fill(order.begin(), order.end(), 0);
        nfailed.store(0);
        ++epoch;
        cv_go.notify_all();
        cv_done.wait(lock, [&] { return left == 0; });
    }
    // status of the rank that failed first, its text behind "rank k: "
    int verdict() {
        int first = -1;
        for (int k = 0; k < P; ++k)
            if (rc[k] != MGN_OK && (first < 0 || order[k] < order[first])) first = k;
        if (first < 0) return MGN_OK;
        const char* t = h[first] ? mgn_last_error(h[first]) : "no handle";
        err = "rank " + std::to_string(first) + ": " + (t ? t : "");
        return rc[first];
    }
    // a fresh communicator on every rank (at creation, and after a failed call: the old one may have been aborted)
    int connect() {
        if (P == 1) return MGN_OK;
        if (int r = mgn_comm_unique_id(id, MGN_COMM_LOCAL)) { err = mgn_last_error(nullptr); return r; }
        have_comm = true;
        dispatch([this](int k) {
            (void)mgn_comm_destroy(h[k]);
            return mgn_comm_init(h[k], id, MGN_COMM_ID_BYTES, MGN_COMM_LOCAL);
        }, -1);
        return verdict();
    }
    // every rank runs f(rank, handle); on failure the communicator is replaced before the status goes back
    int run(const std::function<int(int, mgn_handle*)>& f) {
        dispatch([&](int k) { return f(k, h[k]); }, -1);
        const int r = verdict();
        if (r != MGN_OK && P > 1) {
            const std::string keep = err;
            if (connect() != MGN_OK) err = keep + " (and the communicator could not be rebuilt: " + err + ")";
            else err = keep;
        }
        return r;
    }
    template <typename T>
    T* out_of(int k, T* callers, size_t count) {       // rank 0: the caller's buffer; the others: scratch of the same size
        if (k == 0 || !callers) return callers;
        if (scratch[k].size() < count * sizeof(T)) scratch[k].resize(count * sizeof(T));
        return reinterpret_cast<T*>(scratch[k].data());
    }
    // A call with up to three float outputs.  out_of hands out the START of the rank's scratch, so two uses in one call would alias and
    // the second could move the first: here the pieces lie one behind the other in one allocation.  A NULL of the caller stays NULL.
    struct Outs { float* p[3]; };
    Outs outs_of(int k, float* c0, size_t n0, float* c1, size_t n1, float* c2 = nullptr, size_t n2 = 0) {
        if (k == 0) return Outs{{c0, c1, c2}};
        float* const callers[3] = {c0, c1, c2};
        const size_t counts[3] = {n0, n1, n2};
        size_t total = 0;
        for (int i = 0; i < 3; ++i) total += callers[i] ? counts[i] : 0;
        float* base = out_of<float>(k, c0 ? c0 : (c1 ? c1 : c2), total);
        Outs o{};
        size_t off = 0;
        for (int i = 0; i < 3; ++i) {
            o.p[i] = callers[i] ? base + off : nullptr;
            off += callers[i] ? counts[i] : 0;
        }
        return o;
    }
};
#pragma GCC visibility pop

namespace {
thread_local std::string g_group_create_error;   // like g_create_error (mgn_api.cpp): a failed create reports to its own thread
int create_fail(int code, const std::string& what) {
    g_group_create_error = what;
    return code;
}
int gfail(mgn_group* g, int code, const char* what) {
    if (g) g->err = what;
    return code;
}
}  // namespace

extern "C" {

int mgn_group_create(const mgn_config* cfg, int32_t nranks, const int32_t* devices, mgn_group** out) try {
    if (!out) return create_fail(MGN_E_ARG, "mgn_group_create: null out pointer");
    *out = nullptr;
    if (!cfg || !devices) return create_fail(MGN_E_ARG, "mgn_group_create: null argument");
    if (nranks < 1 || nranks > mgn::COMM_MAX_RANKS) return create_fail(MGN_E_ARG, "mgn_group_create: nranks must be 1 .. 64");
    int none = 0;
    for (int k = 0; k < nranks; ++k) {
        if (devices[k] < 0 && devices[k] != MGN_DEVICE_NONE) return create_fail(MGN_E_ARG, "mgn_group_create: devices[] holds HIP ordinals (or MGN_DEVICE_NONE for every rank)");
        none += devices[k] == MGN_DEVICE_NONE;
    }
    if (none != 0 && none != nranks) return create_fail(MGN_E_ARG, "mgn_group_create: MGN_DEVICE_NONE for some ranks only");
    // single-partition modes: answered here, not deep inside a rank
    if (nranks > 1 && cfg->n_edge_sets == 2) return create_fail(MGN_E_UNSUPPORTED, "mgn_group_create: two edge sets run on one partition");
    if (nranks > 1 && cfg->ln_dims == MGN_LN_ALL) return create_fail(MGN_E_UNSUPPORTED, "mgn_group_create: ln_dims = MGN_LN_ALL (whole-array LayerNorm) runs on one partition");
    std::unique_ptr<mgn_group> g(new mgn_group());
    g->cfg = *cfg;
    g->P = nranks;
    g->host_only = none != 0;
    g->devices.assign(devices, devices + nranks);
    g->h.assign(nranks, nullptr);
    g->rc.assign(nranks, MGN_OK);
    g->order.assign(nranks, 0);
    g->scratch.resize(nranks);
    for (int k = 0; k < nranks; ++k) g->workers.emplace_back([p = g.get(), k] { p->work(k); });
    int rc = MGN_OK;
    std::string why;
    for (int k = 0; k < nranks && rc == MGN_OK; ++k) {   // one at a time: the text of a failed mgn_create is process-wide
        g->dispatch([&](int r) {
            mgn_config c = g->cfg;
            c.rank = r;
            c.nranks = nranks;
            c.device = g->devices[r];
            const int e = mgn_create(&c, &g->h[r]);
            if (e != MGN_OK) why = "rank " + std::to_string(r) + ": " + mgn_last_error(nullptr);
            return e;
        }, k);
        rc = g->rc[k];
    }
    if (rc == MGN_OK && (rc = g->connect()) != MGN_OK) why = g->err;
    if (rc != MGN_OK) {
        mgn_group_destroy(g.release());
        return create_fail(rc, "mgn_group_create: " + why);
    }
    *out = g.release();
    return MGN_OK;
} catch (...) { return create_fail(MGN_E_OOM, "mgn_group_create: host allocation failed"); }

void mgn_group_destroy(mgn_group* g) {
    if (!g) return;
    try {
        if (!g->workers.empty()) {
            g->dispatch([g](int k) {                  // each rank's handle goes where it was made and used
                if (g->h[k]) mgn_destroy(g->h[k]);
                g->h[k] = nullptr;
                return MGN_OK;
            }, -1);
        }
    } catch (...) {
    }
    {
        std::lock_guard<std::mutex> lock(g->mu);
        g->quit = true;
    }
    g->cv_go.notify_all();
    for (std::thread& t : g->workers)
        if (t.joinable()) t.join();
    delete g;
}

const char* mgn_group_last_error(const mgn_group* g) { return g ? g->err.c_str() : g_group_create_error.c_str(); }

mgn_handle* mgn_group_rank_handle(mgn_group* g, int32_t rank) { return g && rank >= 0 && rank < g->P ? g->h[rank] : nullptr; }

#define GROUP_TRY(g) if (!(g)) return MGN_E_ARG; try
#define GROUP_CATCH(g) catch (...) { return gfail(g, MGN_E_OOM, "mgn_group: host allocation failed"); }

int mgn_group_set_params(mgn_group* g, const float* packed, size_t n) {
    GROUP_TRY(g) { return g->run([&](int, mgn_handle* h) { return mgn_set_params(h, packed, n); }); } GROUP_CATCH(g)
}

int mgn_group_set_norms(mgn_group* g, const float* ns, const float* nsh, const float* es, const float* esh, const float* os, const float* osh) {
    GROUP_TRY(g) { return g->run([&](int, mgn_handle* h) { return mgn_set_norms(h, ns, nsh, es, esh, os, osh); }); } GROUP_CATCH(g)
}

int mgn_group_set_graph(mgn_group* g, int32_t N, int64_t E, const int32_t* senders, const int32_t* receivers, int32_t index_base,
                        const float* mesh_pos, int32_t pos_dim) {
    GROUP_TRY(g) {
        const int rc = g->run([&](int, mgn_handle* h) { return mgn_set_graph(h, N, E, senders, receivers, index_base, mesh_pos, pos_dim); });
        if (rc == MGN_OK) g->N = N;
        return rc;
    } GROUP_CATCH(g)
}

int mgn_group_set_static(mgn_group* g, const float* onehot, const float* ef_raw, const float* val_mask) {
    GROUP_TRY(g) { return g->run([&](int, mgn_handle* h) { return mgn_set_static(h, onehot, ef_raw, val_mask); }); } GROUP_CATCH(g)
}

int mgn_group_forward(mgn_group* g, const float* nf, const float* ef, float* out) {
    GROUP_TRY(g) {
        const size_t n = (size_t)g->N * g->cfg.O;
        return g->run([&](int k, mgn_handle* h) { return mgn_forward(h, nf, ef, g->out_of(k, out, n)); });
    } GROUP_CATCH(g)
}

int mgn_group_ode_step(mgn_group* g, const float* x, const float* onehot, const float* ef_raw, const float* val_mask, float* dxdt) {
    GROUP_TRY(g) {
        const size_t n = (size_t)g->N * g->cfg.O;
        return g->run([&](int k, mgn_handle* h) { return mgn_ode_step(h, x, onehot, ef_raw, val_mask, g->out_of(k, dxdt, n)); });
    } GROUP_CATCH(g)
}

extern "C++" {
namespace {
// mgn_group_rollout (tab null) and mgn_group_rollout_erk (its tableau and step mode)
int group_rollout(mgn_group* g, const char* who, mgn_rollout_desc* d, const double* tab, int32_t adaptive) {
    if (!d) return gfail(g, MGN_E_ARG, (std::string(who) + ": null argument").c_str());
    const size_t n = (size_t)(d->n_saves > 0 ? d->n_saves : 0) * g->N * g->cfg.O;
    std::vector<mgn_rollout_desc> ds(g->P, *d);         // every rank fills its own counters; rank 0's go back
    const int rc = g->run([&](int k, mgn_handle* h) {
        ds[k].out = g->out_of(k, d->out, n);
        return tab ? mgn_rollout_erk(h, &ds[k], tab, adaptive) : mgn_rollout(h, &ds[k]);
    });
    d->n_accept = ds[0].n_accept;
    d->n_reject = ds[0].n_reject;
    d->n_rhs = ds[0].n_rhs;
    return rc;
}
}  // namespace
}

int mgn_group_rollout(mgn_group* g, mgn_rollout_desc* d) {
    GROUP_TRY(g) { return group_rollout(g, "mgn_group_rollout", d, nullptr, 0); } GROUP_CATCH(g)
}

int mgn_group_rollout_erk(mgn_group* g, mgn_rollout_desc* d, const double* tab, int32_t adaptive) {
    GROUP_TRY(g) {
        if (mgn_erk_check(tab) != MGN_OK) return gfail(g, MGN_E_ARG, "mgn_group_rollout_erk: the tableau does not pass mgn_erk_check");
        return group_rollout(g, "mgn_group_rollout_erk", d, tab, adaptive);
    } GROUP_CATCH(g)
}

int mgn_group_step(mgn_group* g, const float* nf, const float* ef, const float* target, const int32_t* mask, int64_t nmask,
                   int32_t mask_index_base, float* grads, size_t n_grads, float* loss) {
    GROUP_TRY(g) {
        std::vector<float> losses(g->P, 0.f);
        return g->run([&](int k, mgn_handle* h) {
            return mgn_step(h, nf, ef, target, mask, nmask, mask_index_base, g->out_of(k, grads, n_grads), n_grads,
                            k == 0 || !loss ? loss : &losses[k]);
        });
    } GROUP_CATCH(g)
}

// The datapoint family: the same call on every rank (the nranks > 1 contract of mgn_step_datapoint; a group of one is the plain handle).
int mgn_group_train_set_trajectory(mgn_group* g, const float* frames, int32_t T, const float* times, float dt, const float* node_type_onehot,
                                   const float* ef_raw) {
    GROUP_TRY(g) { return g->run([&](int, mgn_handle* h) { return mgn_train_set_trajectory(h, frames, T, times, dt, node_type_onehot, ef_raw); }); } GROUP_CATCH(g)
}

int mgn_group_train_set_noise(mgn_group* g, const float* stddev, const uint8_t* noisy, uint64_t seed) {
    GROUP_TRY(g) { return g->run([&](int, mgn_handle* h) { return mgn_train_set_noise(h, stddev, noisy, seed); }); } GROUP_CATCH(g)
}

int mgn_group_train_online_norms(mgn_group* g, int32_t node_on, int32_t edge_on, int32_t out_on, double max_accumulations, float std_epsilon) {
    GROUP_TRY(g) {
        return g->run([&](int, mgn_handle* h) { return mgn_train_online_norms(h, node_on, edge_on, out_on, max_accumulations, std_epsilon); });
    } GROUP_CATCH(g)
}

// read: rank 0's totals (every rank holds the same bits); write: the same values on every rank
int mgn_group_train_norm_state(mgn_group* g, int32_t group, int32_t write, double* sum, double* sum_squares, double* count_and_calls) {
    GROUP_TRY(g) {
        const size_t dim = group == 1 ? (size_t)g->cfg.Fe : (size_t)g->cfg.O;
        std::vector<double> sink((size_t)g->P * (2 * dim + 2), 0.0);       // what the ranks other than 0 read
        return g->run([&](int k, mgn_handle* h) {
            if (write || k == 0) return mgn_train_norm_state(h, group, write, sum, sum_squares, count_and_calls);
            double* s = sink.data() + (size_t)k * (2 * dim + 2);
            return mgn_train_norm_state(h, group, 0, s, s + dim, s + 2 * dim);
        });
    } GROUP_CATCH(g)
}

int mgn_group_step_datapoint(mgn_group* g, int32_t datapoint, int32_t accumulate, const int32_t* mask, int64_t nmask, int32_t mask_index_base,
                             float* grads, size_t n_grads, float* loss) {
    GROUP_TRY(g) {
        std::vector<float> losses(g->P, 0.f);
        return g->run([&](int k, mgn_handle* h) {
            return mgn_step_datapoint(h, datapoint, accumulate, mask, nmask, mask_index_base, g->out_of(k, grads, n_grads), n_grads,
                                      k == 0 || !loss ? loss : &losses[k]);
        });
    } GROUP_CATCH(g)
}

// every rank writes the rows of its own nodes and edges into the caller's arrays: disjoint rows, complete arrays
int mgn_group_datapoint_export(mgn_group* g, int32_t datapoint, int32_t normalised, float* nf, float* ef, float* target) {
    GROUP_TRY(g) { return g->run([&](int, mgn_handle* h) { return mgn_datapoint_export(h, datapoint, normalised, nf, ef, target); }); } GROUP_CATCH(g)
}

// Solver-based training and the validation rollout on the partitioned mesh: the drivers behind the rank-handle symbols of the same
// names, told to serve partitions (the symbols themselves keep refusing them).  Every rank is handed the caller's GLOBAL host arrays
// and returns the complete result; rank 0 writes the caller's buffers, descriptors and counters.  A group of one is the plain call.
extern "C++" {
namespace {
// the driver's C++ exceptions end here, as MGN_CATCH ends them in the rank-handle symbols
template <typename F> int guarded(mgn_handle* h, F&& f) try { return f(); } MGN_CATCH(h)
}  // namespace
}

int mgn_group_ode_vjp(mgn_group* g, const float* x, const float* node_type_onehot, const float* ef_raw, const float* val_mask, const float* lambda,
                      float* dxdt, float* xbar, float* grads, size_t n_grads) {
    GROUP_TRY(g) {
        const size_t n = (size_t)g->N * g->cfg.O;
        return g->run([&](int k, mgn_handle* h) {
            return guarded(h, [&] {
                const mgn_group::Outs o = g->outs_of(k, dxdt, n, xbar, n, grads, n_grads);
                return mgn::ode_vjp_run(h, x, node_type_onehot, ef_raw, val_mask, lambda, o.p[0], o.p[1], o.p[2], n_grads, true);
            });
        });
    } GROUP_CATCH(g)
}

int mgn_group_forward_vjp(mgn_group* g, const float* nf, const float* ef, const float* ybar, float* out, float* nfbar, float* grads, size_t n_grads) {
    GROUP_TRY(g) {
        const size_t N = (size_t)g->N;
        return g->run([&](int k, mgn_handle* h) {
            return guarded(h, [&] {
                const mgn_group::Outs o = g->outs_of(k, out, N * g->cfg.O, nfbar, N * g->cfg.Fn, grads, n_grads);
                return mgn::forward_vjp_run(h, nf, ef, ybar, o.p[0], o.p[1], o.p[2], n_grads, true);
            });
        });
    } GROUP_CATCH(g)
}

extern "C++" {
namespace {
// mgn_group_solver_grad (o null) and mgn_group_solver_grad_tsit5: every rank its own copy of the descriptors (counters, the step record),
// rank 0's go back
int group_solver_grad(mgn_group* g, const char* who, mgn_rollout_desc* d, mgn_solver_grad_opts* o, bool tsit5, const float* gt, const float* loss_scale,
                      const float* cont_target, float cont_weight, float* grads, size_t n_grads, float* loss) {
    if (!d || (tsit5 && !o)) return gfail(g, MGN_E_ARG, (std::string(who) + ": null argument").c_str());
    const size_t n = (size_t)(d->n_saves > 0 ? d->n_saves : 0) * g->N * g->cfg.O;
    const size_t cap = o && o->step_cap > 0 ? (size_t)o->step_cap : 0;
    std::vector<mgn_rollout_desc> ds(g->P, *d);
    std::vector<mgn_solver_grad_opts> os(g->P, o ? *o : mgn_solver_grad_opts{});
    std::vector<std::vector<double>> rec(g->P);          // the step records of the ranks other than 0
    std::vector<float> losses(g->P, 0.f);
    const int rc = g->run([&](int k, mgn_handle* h) {
        return guarded(h, [&] {
            const mgn_group::Outs outs = g->outs_of(k, d->out, n, grads, n_grads);
            ds[k].out = outs.p[0];
            if (o && k > 0) {
                rec[k].assign(2 * cap, 0.0);
                if (o->step_t) os[k].step_t = rec[k].data();
                if (o->step_h) os[k].step_h = rec[k].data() + cap;
            }
            return mgn::solver_grad_run(h, &ds[k], o ? &os[k] : nullptr, tsit5, gt, loss_scale, cont_target, cont_weight, outs.p[1], n_grads,
                                        k == 0 || !loss ? loss : &losses[k], true);
        });
    });
    d->n_accept = ds[0].n_accept;
    d->n_reject = ds[0].n_reject;
    d->n_rhs = ds[0].n_rhs;
    if (o) {
        o->n_steps = os[0].n_steps;
        o->stored_bytes = os[0].stored_bytes;
    }
    return rc;
}
}  // namespace
}

int mgn_group_solver_grad(mgn_group* g, mgn_rollout_desc* d, const float* gt, const float* loss_scale, const float* cont_target, float cont_weight,
                          float* grads, size_t n_grads, float* loss) {
    GROUP_TRY(g) {
        return group_solver_grad(g, "mgn_group_solver_grad", d, nullptr, false, gt, loss_scale, cont_target, cont_weight, grads, n_grads, loss);
    } GROUP_CATCH(g)
}

int mgn_group_solver_grad_tsit5(mgn_group* g, mgn_rollout_desc* d, mgn_solver_grad_opts* o, const float* gt, const float* loss_scale,
                                const float* cont_target, float cont_weight, float* grads, size_t n_grads, float* loss) {
    GROUP_TRY(g) {
        return group_solver_grad(g, "mgn_group_solver_grad_tsit5", d, o, true, gt, loss_scale, cont_target, cont_weight, grads, n_grads, loss);
    } GROUP_CATCH(g)
}

extern "C++" {
namespace {
// mgn_group_rollout_eval (tab null) and mgn_group_rollout_eval_erk (its tableau and step mode)
int group_rollout_eval(mgn_group* g, const char* who, mgn_rollout_desc* d, mgn_rollout_eval_desc* e, const double* tab, int32_t adaptive) {
    if (!d || !e) return gfail(g, MGN_E_ARG, (std::string(who) + ": null argument").c_str());
    const size_t no = (size_t)g->N * g->cfg.O, ns = (size_t)(d->n_saves > 0 ? d->n_saves : 0);
    std::vector<mgn_rollout_desc> ds(g->P, *d);
    std::vector<mgn_rollout_eval_desc> es(g->P, *e);
    std::vector<std::vector<double>> ms(g->P);       // mse_save of the ranks other than 0 (doubles; the float outputs share the scratch)
    const int rc = g->run([&](int k, mgn_handle* h) {
        return guarded(h, [&] {
            if (k > 0) {      // d->out [n_saves][N][O], then mse_time [N][O], in this rank's scratch
                const mgn_group::Outs o = g->outs_of(k, d->out, ns * no, e->mse_time, no);
                ds[k].out = o.p[0];
                es[k].mse_time = o.p[1];
                if (e->mse_save) {
                    ms[k].assign(ns * g->cfg.O, 0.0);
                    es[k].mse_save = ms[k].data();
                }
            }
            return mgn::rollout_eval_run(h, &ds[k], &es[k], true, tab, adaptive);
        });
    });
    d->n_accept = ds[0].n_accept;
    d->n_reject = ds[0].n_reject;
    d->n_rhs = ds[0].n_rhs;
    e->val_loss = es[0].val_loss;
    return rc;
}
}  // namespace
}

int mgn_group_rollout_eval(mgn_group* g, mgn_rollout_desc* d, mgn_rollout_eval_desc* e) {
    GROUP_TRY(g) { return group_rollout_eval(g, "mgn_group_rollout_eval", d, e, nullptr, 0); } GROUP_CATCH(g)
}

int mgn_group_rollout_eval_erk(mgn_group* g, mgn_rollout_desc* d, mgn_rollout_eval_desc* e, const double* tab, int32_t adaptive) {
    GROUP_TRY(g) {
        if (mgn_erk_check(tab) != MGN_OK) return gfail(g, MGN_E_ARG, "mgn_group_rollout_eval_erk: the tableau does not pass mgn_erk_check");
        return group_rollout_eval(g, "mgn_group_rollout_eval_erk", d, e, tab, adaptive);
    } GROUP_CATCH(g)
}

int mgn_group_latents_randn(mgn_group* g, uint64_t seed) {
    GROUP_TRY(g) { return g->run([&](int, mgn_handle* h) { return mgn_latents_randn(h, seed); }); } GROUP_CATCH(g)
}

int mgn_group_processor_steps_dev(mgn_group* g, int32_t nsteps) {
    GROUP_TRY(g) { return g->run([&](int, mgn_handle* h) { return mgn_processor_steps_dev(h, nsteps); }); } GROUP_CATCH(g)
}

int mgn_group_latents_checksum(mgn_group* g, double* sum_v, double* sum_e, double* sumsq_v, double* sumsq_e) {
    GROUP_TRY(g) {
        std::vector<double> part((size_t)4 * g->P, 0.0);
        const int rc = g->run([&](int k, mgn_handle* h) {
            double* p = part.data() + (size_t)4 * k;
            return mgn_latents_checksum(h, p, p + 1, p + 2, p + 3);
        });
        if (rc != MGN_OK) return rc;
        double acc[4] = {0, 0, 0, 0};
        for (int k = 0; k < g->P; ++k)                       // ascending rank order: repeatable
            for (int i = 0; i < 4; ++i) acc[i] += part[(size_t)4 * k + i];
        if (sum_v) *sum_v = acc[0];
        if (sum_e) *sum_e = acc[1];
        if (sumsq_v) *sumsq_v = acc[2];
        if (sumsq_e) *sumsq_e = acc[3];
        return MGN_OK;
    } GROUP_CATCH(g)
}

int mgn_group_synchronize(mgn_group* g) {
    GROUP_TRY(g) { return g->run([&](int, mgn_handle* h) { return mgn_synchronize(h); }); } GROUP_CATCH(g)
}

}  // extern "C"
