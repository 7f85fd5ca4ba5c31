// mgn_group: one handle that drives the P partitions of a mesh from one caller thread (include/mgn_hip.h, "one process, P partitions").
// Inside it is what the tests' thread-ranks are: one worker thread per rank, each owning an ordinary rank handle, joined by one
// MGN_COMM_LOCAL communicator (comm.cpp).  A group call is the same mgn_* call on every worker.
// A replica group (mgn_group_create_replicas) is the same machinery around P whole copies of the model: every handle is rank 0 of 1,
// the communicator is the group's own, and mgn_group_step_datapoints splits a minibatch over the replicas (below).
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
    // A replica group (mgn_group_create_replicas): every handle is a whole one-partition handle (rank 0 of 1), and the communicator that
    // joins them belongs to the group, one end per worker -- the handles themselves have none.
    bool replicas = false;
    std::vector<mgn::Comm*> rcomm;
    std::vector<std::shared_ptr<std::mutex>> turn;   // [rank]: shared by the replicas on one device (run())
    // mgn_group_step_datapoints, per rank, on the rank's device: res the gradient the call leaves (what mgn_group_adam_update(NULL) reads);
    // replica groups of more than one: share, the replica's own gradient as it goes into the gather, and all, the gathered [P][stride]
    struct RankBufs { DevBuf res, share, all; };
    std::unique_ptr<RankBufs[]> bufs;
    bool have_grad = false;                          // res holds the gradient of a successful mgn_group_step_datapoints

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
        if (replicas) {
            dispatch([this](int k) {
                delete rcomm[k];
                std::string why;
                rcomm[k] = mgn::comm_create(id, MGN_COMM_LOCAL, k, P, !host_only, why);
                return rcomm[k] ? MGN_OK : mgn::fail(h[k], MGN_E_RCCL, "the replicas' communicator: %s", why.c_str());
            }, -1);
            return verdict();
        }
        dispatch([this](int k) {
            (void)mgn_comm_destroy(h[k]);
            return mgn_comm_init(h[k], id, MGN_COMM_ID_BYTES, MGN_COMM_LOCAL);
        }, -1);
        return verdict();
    }
    // every rank runs f(rank, handle); on failure the communicator is replaced before the status goes back.
    // Replicas that share a device take turns (turn[k]: one mutex per distinct ordinal) unless f holds a collective, which needs all of
    // them inside at once.  A replica is a one-partition handle, and those capture and replay hipGraphs with parallel branches (the
    // training step's second stream, the small-mesh inference passes); partitions run eagerly.  Two workers capturing on one device at
    // the same time have ended in a segmentation fault inside a worker thread (docs/experiments.md), so a device's graph capture,
    // instantiation and replay are entered by one thread at a time.  Replicas on different devices do not wait for each other.
    int run(const std::function<int(int, mgn_handle*)>& f, bool collective = false) {
        dispatch([&](int k) {
            if (!replicas || collective || !turn[k]) return f(k, h[k]);
            std::lock_guard<std::mutex> mine(*turn[k]);
            return f(k, h[k]);
        }, -1);
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

// A replica group: mgn_group_create's workers and dispatch around P whole copies of the model (every handle rank 0 of 1, so the
// single-partition modes are legal), joined by a communicator of the group's own (mgn_group::connect).
int mgn_group_create_replicas(const mgn_config* cfg, int32_t nreplicas, const int32_t* devices, mgn_group** out) try {
    const char* who = "mgn_group_create_replicas";
    if (!out) return create_fail(MGN_E_ARG, std::string(who) + ": null out pointer");
    *out = nullptr;
    if (!cfg || !devices) return create_fail(MGN_E_ARG, std::string(who) + ": null argument");
    if (nreplicas < 1 || nreplicas > mgn::COMM_MAX_RANKS) return create_fail(MGN_E_ARG, std::string(who) + ": nreplicas must be 1 .. 64");
    static_assert(mgn::REPLICA_FOLD_MAX == mgn::COMM_MAX_RANKS, "the fold's weight table holds the communicator's largest group");
    int none = 0;
    for (int k = 0; k < nreplicas; ++k) {
        if (devices[k] < 0 && devices[k] != MGN_DEVICE_NONE)
            return create_fail(MGN_E_ARG, std::string(who) + ": devices[] holds HIP ordinals (or MGN_DEVICE_NONE for every replica)");
        none += devices[k] == MGN_DEVICE_NONE;
    }
    if (none != 0 && none != nreplicas) return create_fail(MGN_E_ARG, std::string(who) + ": MGN_DEVICE_NONE for some replicas only");
    std::unique_ptr<mgn_group> g(new mgn_group());
    g->cfg = *cfg;
    g->P = nreplicas;
    g->replicas = true;
    g->host_only = none != 0;
    g->devices.assign(devices, devices + nreplicas);
    g->h.assign(nreplicas, nullptr);
    g->rcomm.assign(nreplicas, nullptr);
    g->turn.assign(nreplicas, nullptr);
    for (int k = 0; k < nreplicas; ++k) {                 // one turn-taking mutex per distinct device (mgn_group::run)
        for (int j = 0; j < k && !g->turn[k]; ++j)
            if (devices[j] == devices[k]) g->turn[k] = g->turn[j];
        if (!g->turn[k]) g->turn[k] = std::make_shared<std::mutex>();
    }
    g->rc.assign(nreplicas, MGN_OK);
    g->order.assign(nreplicas, 0);
    g->scratch.resize(nreplicas);
    for (int k = 0; k < nreplicas; ++k) g->workers.emplace_back([p = g.get(), k] { p->work(k); });
    int rc = MGN_OK;
    std::string why;
    for (int k = 0; k < nreplicas && rc == MGN_OK; ++k) {   // one at a time: the text of a failed mgn_create is process-wide
        g->dispatch([&](int r) {
            mgn_config c = g->cfg;
            c.rank = 0;
            c.nranks = 1;
            c.device = g->devices[r];
            const int e = mgn_create(&c, &g->h[r]);
            if (e != MGN_OK) why = "replica " + std::to_string(r) + ": " + mgn_last_error(nullptr);
            return e;
        }, k);
        rc = g->rc[k];
    }
    if (rc == MGN_OK && (rc = g->connect()) != MGN_OK) why = g->err;
    if (rc != MGN_OK) {
        mgn_group_destroy(g.release());
        return create_fail(rc, std::string(who) + ": " + why);
    }
    *out = g.release();
    return MGN_OK;
} catch (...) { return create_fail(MGN_E_OOM, "mgn_group_create_replicas: host allocation failed"); }

void mgn_group_destroy(mgn_group* g) {
    if (!g) return;
    try {
        if (!g->workers.empty()) {
            g->dispatch([g](int k) {                  // each rank's handle goes where it was made and used
                if (g->bufs) { g->bufs[k].res.release(); g->bufs[k].share.release(); g->bufs[k].all.release(); }
                if (k < (int)g->rcomm.size()) { delete g->rcomm[k]; g->rcomm[k] = nullptr; }
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
            return mgn::solver_grad_run(h, &ds[k], o ? &os[k] : nullptr, tsit5 ? MGN_SOLVER_TSIT5 : MGN_SOLVER_EULER, gt, loss_scale, cont_target, cont_weight, outs.p[1], n_grads,
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
        for (int k = 0; k < (g->replicas ? 1 : g->P); ++k)   // ascending rank order: repeatable (replicas hold the same latents: replica 0's sums)
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

// ---- a minibatch of datapoints over the group, and Adam in place (include/mgn_hip_replica.h) ----
// Replica group of P > 1: the list is split into contiguous chunks in listed order (replica k: B_k = B / P + (k < B % P) entries from
// k (B / P) + min(k, B % P)); every replica runs the plain handle call on its chunk with a device buffer of the group's as grads, one
// allgather brings all of them to every replica and launch_replica_fold writes their weighted sum into the rank's resident buffer.
// Everything else (one replica, a partition group) is the handle call itself with the resident buffer as grads.
// Every check is made here, on the caller's thread and for every rank, before a worker is woken: no rank can be left in a collective by
// a refusal.  A share that fails behind the checks (an allocation) ends the call before the gather is entered; a failure inside the gather
// releases the peers through the group's abort, as everywhere.
int mgn_group_step_datapoints(mgn_group* g, const int32_t* datapoints, int32_t B, int32_t accumulate, const int32_t* mask, int64_t nmask,
                              int32_t mask_index_base, float* grads, size_t n_grads, float* loss, float* losses) {
    GROUP_TRY(g) {
        const char* who = "mgn_group_step_datapoints";
        if (!datapoints || !mask || !loss) return gfail(g, MGN_E_ARG, "mgn_group_step_datapoints: null argument");
        if (B < 1) return gfail(g, MGN_E_ARG, "mgn_group_step_datapoints: B must be at least 1");
        const int P = g->P;
        const bool split = g->replicas && P > 1;
        if (!g->replicas && P > 1 && B > 1) return gfail(g, MGN_E_STATE, "mgn_group_step_datapoints with B > 1 drives one partition (or a replica group)");
        const int32_t q = split ? B / P : B, r = split ? B % P : 0;
        const int32_t share = q + (r > 0 ? 1 : 0);                      // the largest share: its rule is the call's
        if (share > MGN_DATAPOINT_BATCH_MAX)
            return gfail(g, MGN_E_ARG, ("mgn_group_step_datapoints: a share of " + std::to_string(share) + " datapoints is more than MGN_DATAPOINT_BATCH_MAX").c_str());
        for (int k = 0; k < P; ++k)
            if (const int rc = mgn::step_datapoints_check(g->h[k], who, datapoints, B, share, mask, nmask, mask_index_base, n_grads)) {
                g->err = "rank " + std::to_string(k) + ": " + mgn_last_error(g->h[k]);
                return rc;
            }
        if (!g->bufs) g->bufs.reset(new mgn_group::RankBufs[P]);
        g->have_grad = false;
        std::vector<float> own_losses;
        float* const L = losses ? losses : (own_losses.assign((size_t)B, 0.f), own_losses.data());
        const size_t n = n_grads, stride = (size_t)mgn::replica_fold_stride((int64_t)n);
        mgn::ReplicaFoldW w{};
        uint64_t active = 0;
        auto first_of = [&](int k) { return k * q + (k < r ? k : r); };
        auto count_of = [&](int k) { return split ? q + (k < r ? 1 : 0) : B; };
        for (int k = 0; split && k < P; ++k)
            if (count_of(k) > 0) {
                w.w[k] = (double)count_of(k) / (double)B;
                active |= (uint64_t)1 << k;
            }
        float mean0 = 0.f;                                               // rank 0's, where the handle call takes the whole list
        const int rc = g->run([&](int k, mgn_handle* h) {
            return guarded(h, [&]() -> int {
                mgn_group::RankBufs& rb = g->bufs[k];
                HIPCHK(h, rb.res.ensure(stride * 4));
                float* gk = rb.res.as<float>();
                if (split) {
                    HIPCHK(h, rb.share.ensure(stride * 4));
                    HIPCHK(h, rb.all.ensure((size_t)P * stride * 4));
                    gk = rb.share.as<float>();
                    // accumulate first, normalise afterwards: all B, in listed order, on every replica; the share then runs without
                    if (accumulate)
                        for (int32_t b = 0; b < B; ++b)
                            if (int e = mgn::datapoint_accumulate(h, datapoints[b])) return e;
                }
                const int32_t acc = split ? 0 : accumulate, s0 = split ? first_of(k) : 0, Bk = count_of(k);
                float mean = 0.f, one = 0.f;                             // (ranks other than 0 of a partition group compute the same loss)
                float* const Lk = split || k == 0 ? L + s0 : &one;
                int e = MGN_OK;
                if (Bk == 1) e = mgn_step_datapoint(h, datapoints[s0], acc, mask, nmask, mask_index_base, gk, n, Lk);
                else if (Bk > 1) e = mgn_step_datapoints(h, datapoints + s0, Bk, acc, mask, nmask, mask_index_base, gk, n, &mean, Lk);
                if (e != MGN_OK) return e;
                if (k == 0) mean0 = mean;
                if (split) return MGN_OK;                                // (the gather is the second phase)
                if (k == 0 && grads) HIPCHK(h, hipMemcpyAsync(grads, rb.res.p, n * 4, hipMemcpyDefault, h->stream));
                HIPCHK(h, hipStreamSynchronize(h->stream));
                return MGN_OK;
            });
        });
        if (rc != MGN_OK) return rc;
        // The gather and the fold, every replica at once: launches and event calls only, what the ranks of a partition group issue side
        // by side.  The shares above ran under mgn_group::run's turns (replicas that share a device), so they come as a phase of their own.
        if (split) {
            const int rc2 = g->run([&](int k, mgn_handle* h) {
                return guarded(h, [&]() -> int {
                    mgn_group::RankBufs& rb = g->bufs[k];
                    if (g->rcomm[k]->allgather(rb.share.p, stride * 4, rb.all.p, h->stream) != 0)
                        return mgn::fail(h, MGN_E_RCCL, "%s: allgather of the replicas' gradients: %s", who, g->rcomm[k]->err.c_str());
                    HIPCHK(h, mgn::launch_replica_fold(rb.all.as<float>(), P, (int64_t)n, w, active, rb.res.as<float>(), h->stream));
                    if (k == 0 && grads) HIPCHK(h, hipMemcpyAsync(grads, rb.res.p, n * 4, hipMemcpyDefault, h->stream));
                    HIPCHK(h, hipStreamSynchronize(h->stream));
                    return MGN_OK;
                });
            }, true);
            if (rc2 != MGN_OK) return rc2;
        }
        if (!g->replicas && B > 1) {
            *loss = mean0;                                               // a partition group of one: the plain call
        } else {
            double s = 0.0;
            for (int32_t b = 0; b < B; ++b) s += (double)L[b];
            *loss = (float)(s / (double)B);
        }
        g->have_grad = true;
        return MGN_OK;
    } GROUP_CATCH(g)
}

int mgn_group_set_params_dev(mgn_group* g, const float* packed, size_t n) {
    GROUP_TRY(g) { return g->run([&](int, mgn_handle* h) { return mgn_set_params_dev(h, packed, n); }); } GROUP_CATCH(g)
}

int mgn_group_get_params_dev(mgn_group* g, int32_t rank, float* packed, size_t n) {
    GROUP_TRY(g) {
        if (rank < 0 || rank >= g->P) return gfail(g, MGN_E_ARG, "mgn_group_get_params_dev: rank outside [0, P)");
        g->dispatch([&](int k) { return mgn_get_params_dev(g->h[k], packed, n); }, rank);   // (no collective: this rank alone)
        return g->verdict();
    } GROUP_CATCH(g)
}

int mgn_group_adam_init(mgn_group* g, const mgn_adam_desc* a) {
    GROUP_TRY(g) { return g->run([&](int, mgn_handle* h) { return mgn_adam_init(h, a); }); } GROUP_CATCH(g)
}

// grads NULL: every rank's update reads the gradient the last mgn_group_step_datapoints left on its own device
int mgn_group_adam_update(mgn_group* g, const float* grads, size_t n_grads) {
    GROUP_TRY(g) {
        if (!grads && g->host_only) return gfail(g, MGN_E_HIP, "mgn_group_adam_update: host-only group (MGN_DEVICE_NONE): no compute path");
        if (!grads && !g->have_grad)
            return gfail(g, MGN_E_STATE, "mgn_group_adam_update: no gradient is resident: mgn_group_step_datapoints has not succeeded yet");
        return g->run([&](int k, mgn_handle* h) { return mgn_adam_update(h, grads ? grads : g->bufs[k].res.as<float>(), n_grads); });
    } GROUP_CATCH(g)
}

// read: rank 0's moments and beta_t (every rank holds the same); write: the same values on every rank
int mgn_group_adam_state(mgn_group* g, int32_t write, float* mt, float* vt, double beta_t[2]) {
    GROUP_TRY(g) {
        const size_t n = mgn_param_count(&g->cfg);
        std::vector<double> bt((size_t)2 * g->P, 0.0);
        return g->run([&](int k, mgn_handle* h) {
            if (write || k == 0 || !mt || !vt || !beta_t) return mgn_adam_state(h, write, mt, vt, beta_t);
            const mgn_group::Outs o = g->outs_of(k, mt, n, vt, n);
            return mgn_adam_state(h, 0, o.p[0], o.p[1], &bt[(size_t)2 * k]);
        });
    } GROUP_CATCH(g)
}

}  // extern "C"
