// The ODE solve drivers behind the C ABI (include/mgn_hip.h): mgn_rollout and mgn_rollout_eval (rollout_solve), mgn_solver_grad and
// mgn_solver_grad_tsit5 (solver_grad), mgn_shooting_grad and its companion engines.  Host orchestration only: the time loops, their
// workspaces and the hipGraph replay of the right-hand side, whose launches are mgn_api.cpp's (encode_impl, run_processor, decode_impl);
// the reverse sweeps are mgn_train.cpp's.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>

#include "engine_internal.h"

using namespace mgn;

namespace {

// Tsitouras 5(4) tableau (the method OrdinaryDiffEq.jl calls Tsit5)
const double TS_C[7] = {0.0, 0.161, 0.327, 0.9, 0.9800255409045097, 1.0, 1.0};
const double TS_A[7][6] = {
    {0, 0, 0, 0, 0, 0},
    {0.161, 0, 0, 0, 0, 0},
    {-0.008480655492356989, 0.335480655492357, 0, 0, 0, 0},
    {2.8971530571054935, -6.359448489975075, 4.3622954328695815, 0, 0, 0},
    {5.325864828439257, -11.748883564062828, 7.4955393428898365, -0.09249506636175525, 0, 0},
    {5.86145544294642, -12.92096931784711, 8.159367898576159, -0.071584973281401, -0.028269050394068383, 0},
    {0.09646076681806523, 0.01, 0.4798896504144996, 1.379008574103742, -3.290069515436081, 2.324710524099774}};
const double TS_BT[7] = {-0.00178001105222577714, -0.0008164344596567469, 0.007880878010261995, -0.1447110071732629,
                         0.5823571654525552, -0.45808210592918697, 0.015151515151515152};

// An explicit Runge-Kutta method as the time loops read it: the flat tableau of include/mgn_hip.h (MGN_ERK_TABLEAU_DOUBLES) unpacked.
// beta1 / beta2 are the PI controller's, the defaults 7/(10 p) and 2/(5 p) filled in.
struct Erk {
    int s = 1, p = 1;
    bool fsal = false, embedded = false;
    double beta1 = 0.7, beta2 = 0.4;
    double A[7][7] = {}, b[7] = {}, c[7] = {}, bt[7] = {};
    // the stages whose right-hand side is evaluated on a stage input of the step, which the training form keeps: all, less the FSAL stage
    int active() const { return s - (fsal ? 1 : 0); }
};

enum { ERK_A = 6, ERK_B = 55, ERK_C = 62, ERK_BT = 69 };     // offsets into the flat tableau

// a tableau mgn_erk_check has passed, unpacked
Erk erk_unpack(const double* tab) {
    Erk e;
    e.s = (int)tab[0]; e.p = (int)tab[1]; e.fsal = tab[2] != 0.0; e.embedded = tab[3] != 0.0;
    const bool defaults = tab[4] == 0.0 && tab[5] == 0.0;
    e.beta1 = defaults ? 7.0 / (10 * e.p) : tab[4];
    e.beta2 = defaults ? 2.0 / (5 * e.p) : tab[5];
    for (int i = 0; i < e.s; ++i) {
        for (int j = 0; j < i; ++j) e.A[i][j] = tab[ERK_A + 7 * i + j];
        e.b[i] = tab[ERK_B + i]; e.c[i] = tab[ERK_C + i];
        e.bt[i] = e.embedded ? tab[ERK_BT + i] : 0.0;
    }
    return e;
}

// the flat tableau of a method given by rows (row i of A holds i entries); bt null: no embedded pair
void erk_fill(double* tab, int s, int p, bool fsal, const double* const* rows, const double* b, const double* c, const double* bt, double beta1,
              double beta2) {
    std::fill(tab, tab + MGN_ERK_TABLEAU_DOUBLES, 0.0);
    tab[0] = s; tab[1] = p; tab[2] = fsal ? 1.0 : 0.0; tab[3] = bt ? 1.0 : 0.0; tab[4] = beta1; tab[5] = beta2;
    for (int i = 0; i < s; ++i) {
        for (int j = 0; j < i; ++j) tab[ERK_A + 7 * i + j] = rows[i][j];
        tab[ERK_B + i] = b[i]; tab[ERK_C + i] = c[i];
        if (bt) tab[ERK_BT + i] = bt[i];
    }
}

// Tsit5 as a tableau: TS_A / TS_C / TS_BT above, b = row 7 (FSAL), order 5, the default betas
void erk_fill_tsit5(double* tab) {
    const double* rows[7];
    double b[7] = {};
    for (int i = 0; i < 7; ++i) rows[i] = TS_A[i];
    for (int j = 0; j < 6; ++j) b[j] = TS_A[6][j];
    erk_fill(tab, 7, 5, true, rows, b, TS_C, TS_BT, 0.0, 0.0);
}

}  // namespace

extern "C" int mgn_erk_check(const double* tab) {
    if (!tab) return MGN_E_ARG;
    for (int i = 0; i < MGN_ERK_TABLEAU_DOUBLES; ++i)
        if (!std::isfinite(tab[i])) return MGN_E_ARG;
    for (int i = 0; i < 4; ++i)
        if (tab[i] != std::floor(tab[i])) return MGN_E_ARG;
    if (tab[0] < 1 || tab[0] > MGN_ERK_MAX_STAGES || tab[1] < 1 || tab[1] > 1e6) return MGN_E_ARG;
    if ((tab[2] != 0 && tab[2] != 1) || (tab[3] != 0 && tab[3] != 1)) return MGN_E_ARG;
    if (tab[4] < 0 || tab[5] < 0) return MGN_E_ARG;
    const int s = (int)tab[0];
    const double *A = tab + ERK_A, *b = tab + ERK_B, *c = tab + ERK_C, *bt = tab + ERK_BT;
    double sb = 0.0, sbt = 0.0;
    for (int i = 0; i < s; ++i) {
        for (int j = i; j < s; ++j)
            if (A[7 * i + j] != 0.0) return MGN_E_ARG;       // explicit methods only
        sb += b[i];
        sbt += bt[i];
    }
    if (std::fabs(sb - 1.0) > 1e-10) return MGN_E_ARG;
    if (tab[3] != 0 && std::fabs(sbt) > 1e-10) return MGN_E_ARG;
    if (tab[2] != 0) {         // first same as last: stage s is f(x_{n+1})
        if (b[s - 1] != 0.0 || c[s - 1] != 1.0) return MGN_E_ARG;
        for (int j = 0; j < s; ++j)
            if (A[7 * (s - 1) + j] != b[j]) return MGN_E_ARG;
    }
    return MGN_OK;
}

// The named methods, their coefficients entered as rationals and rounded once (a quotient of two exactly representable integers).
extern "C" int mgn_erk_named(int32_t name, double* tab) {
    if (!tab) return MGN_E_ARG;
    static const double z1[1] = {0};
    switch (name) {
    case MGN_ERK_EULER: {
        const double b[1] = {1}, c[1] = {0};
        const double* rows[1] = {z1};
        erk_fill(tab, 1, 1, false, rows, b, c, nullptr, 0, 0);
        return MGN_OK;
    }
    case MGN_ERK_HEUN: case MGN_ERK_MIDPOINT: case MGN_ERK_RALSTON: {
        const double a21 = name == MGN_ERK_HEUN ? 1.0 : name == MGN_ERK_MIDPOINT ? 1.0 / 2 : 2.0 / 3;
        const double r1[1] = {a21};
        const double* rows[2] = {z1, r1};
        const double bh[2] = {1.0 / 2, 1.0 / 2}, bm[2] = {0, 1}, br[2] = {1.0 / 4, 3.0 / 4};
        const double c[2] = {0, a21};
        erk_fill(tab, 2, 2, false, rows, name == MGN_ERK_HEUN ? bh : name == MGN_ERK_MIDPOINT ? bm : br, c, nullptr, 0, 0);
        return MGN_OK;
    }
    case MGN_ERK_RK4: {
        const double r1[1] = {1.0 / 2}, r2[2] = {0, 1.0 / 2}, r3[3] = {0, 0, 1};
        const double* rows[4] = {z1, r1, r2, r3};
        const double b[4] = {1.0 / 6, 1.0 / 3, 1.0 / 3, 1.0 / 6}, c[4] = {0, 1.0 / 2, 1.0 / 2, 1};
        erk_fill(tab, 4, 4, false, rows, b, c, nullptr, 0, 0);
        return MGN_OK;
    }
    case MGN_ERK_BS3: {
        const double r1[1] = {1.0 / 2}, r2[2] = {0, 3.0 / 4}, b[4] = {2.0 / 9, 1.0 / 3, 4.0 / 9, 0};
        const double* rows[4] = {z1, r1, r2, b};
        const double c[4] = {0, 1.0 / 2, 3.0 / 4, 1}, bt[4] = {-5.0 / 72, 1.0 / 12, 1.0 / 9, -1.0 / 8};
        erk_fill(tab, 4, 3, true, rows, b, c, bt, 0, 0);
        return MGN_OK;
    }
    case MGN_ERK_DP5: {
        const double r1[1] = {1.0 / 5}, r2[2] = {3.0 / 40, 9.0 / 40}, r3[3] = {44.0 / 45, -56.0 / 15, 32.0 / 9};
        const double r4[4] = {19372.0 / 6561, -25360.0 / 2187, 64448.0 / 6561, -212.0 / 729};
        const double r5[5] = {9017.0 / 3168, -355.0 / 33, 46732.0 / 5247, 49.0 / 176, -5103.0 / 18656};
        const double b[7] = {35.0 / 384, 0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84, 0};
        const double* rows[7] = {z1, r1, r2, r3, r4, r5, b};
        const double c[7] = {0, 1.0 / 5, 3.0 / 10, 4.0 / 5, 8.0 / 9, 1, 1};
        const double bt[7] = {71.0 / 57600, 0, -71.0 / 16695, 71.0 / 1920, -17253.0 / 339200, 22.0 / 525, -1.0 / 40};
        erk_fill(tab, 7, 5, true, rows, b, c, bt, 0.17, 0.04);
        return MGN_OK;
    }
    case MGN_ERK_TSIT5:
        erk_fill_tsit5(tab);
        return MGN_OK;
    default:
        return MGN_E_ARG;
    }
}

// Tsit5's dense output, the free 4th-order interpolant of Tsitouras 2011 (what OrdinaryDiffEq.jl evaluates between the steps of a Tsit5
// solve):  x(t_n + theta h) = x_n + h sum_i b_i(theta) k_i,  b_i(theta) = r_i1 theta + r_i2 theta^2 + r_i3 theta^3 + r_i4 theta^4, with
// k_7 = f(x_{n+1}).  b(1) is row 7 of the tableau (b_7(1) = 0).  Host only; the one place the constants live.
extern "C" int mgn_tsit5_interp_weights(double theta, double b[7]) {
    static const double R[7][4] = {{1.0, -2.763706197274826, 2.9132554618219126, -1.0530884977290216},
                                   {0.0, 0.13169999999999998, -0.2234, 0.1017},
                                   {0.0, 3.9302962368947516, -5.941033872131505, 2.490627285651253},
                                   {0.0, -12.411077166933676, 30.33818863028232, -16.548102889244902},
                                   {0.0, 37.50931341651104, -88.1789048947664, 47.37952196281928},
                                   {0.0, -27.896526289197286, 65.09189467479366, -34.87065786149661},
                                   {0.0, 1.5, -4.0, 2.5}};
    if (!b || !(theta >= 0.0 && theta <= 1.0)) return MGN_E_ARG;
    for (int i = 0; i < 7; ++i) b[i] = theta * (R[i][0] + theta * (R[i][1] + theta * (R[i][2] + theta * R[i][3])));
    return MGN_OK;
}

namespace {

// a named method (mgn_erk_named), unpacked
Erk erk_of(int32_t name) {
    double tab[MGN_ERK_TABLEAU_DOUBLES];
    (void)mgn_erk_named(name, tab);
    return erk_unpack(tab);
}
// the tableaux the solvers of mgn_rollout_desc.solver drive: MGN_SOLVER_EULER in training, MGN_SOLVER_TSIT5 everywhere
const Erk& erk_euler() { static const Erk e = erk_of(MGN_ERK_EULER); return e; }
const Erk& erk_tsit5() { static const Erk e = erk_of(MGN_ERK_TSIT5); return e; }

// mgn_rollout's PI controller (beta1, beta2 the tableau's: 7/50 and 2/25 for Tsit5; gamma = 0.9, qmin = 0.2, qmax = 10): the accept /
// reject decision for a trial of size hstep with error estimate EEst, and the next dt (a step cut by a stop does not shrink dt)
struct StepControl {
    static constexpr double gamma = 0.9, qmin = 0.2, qmax = 10.0;
    double beta1, beta2;
    double qold = 1e-4;
    explicit StepControl(const Erk& e) : beta1(e.beta1), beta2(e.beta2) {}
    bool decide(double EEst, double hstep, bool hit_stop, double& dt) {
        const double q11 = std::pow(EEst > 1e-30 ? EEst : 1e-30, beta1);
        if (EEst <= 1.0) {
            double q = q11 / std::pow(qold, beta2);
            q = std::max(1.0 / qmax, std::min(1.0 / qmin, q / gamma));
            qold = std::max(EEst, 1e-4);
            if (!hit_stop || hstep >= dt * (1 - 1e-9)) dt = hstep / q;
            else dt = std::max(dt, hstep / q);
            return true;
        }
        dt = hstep / std::min(1.0 / qmin, q11 / gamma);
        return false;
    }
};

// The time grid of a solve.  The solver's time type (mgn_rollout_desc.time_f64): Float32 times are held in doubles and rounded after
// every operation (a double operation on two floats, rounded to float, IS the float operation).
struct TimeGrid {
    bool f64 = false;
    double t0 = 0.0, t1 = 0.0, dt = 0.0, sdt = 0.0;     // sdt: saves_dt
    explicit TimeGrid(const mgn_rollout_desc* d)
        : f64(d->time_f64 != 0), t0(f64 ? d->t0_f64 : (double)d->t0), t1(f64 ? d->t1_f64 : (double)d->t1),
          dt(f64 ? d->dt_f64 : (double)d->dt), sdt(f64 ? d->saves_dt_f64 : (double)d->saves_dt) {}
    double tt(double v) const { return f64 ? v : (double)(float)v; }
    // the time of save point i
    double stop_time(int i) const { return tt(t0 + (double)i * sdt); }
    // the fixed-step grid: the time after step i of K is the integrator's own t <- t + dt in its time type, step after step (a fixed-step
    // solve has no stops to snap to but the end of the interval); t0 + (i + 1) dt would floor differently at frame boundaries
    double next(int64_t i, int64_t K, double t) const { return (i + 1 == K && std::fabs(tt(t + dt) - t1) <= 1e-5 * sdt) ? t1 : tt(t + dt); }
};

// one call's buffers carved out of one DevBuf: 256-byte aligned offsets, then one ensure of `off` bytes
struct Arena {
    size_t off = 0;
    size_t take(size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; }
};

// the state and stage arrays of a solve, nb bytes each, as offsets into the call's arena, sized by the method: s stage arrays k, the stage
// input utmp (and its copy zs) where there is a stage 2, z7 for an FSAL stage.  fixed: the solve is Rollout::erk_fixed's, which advances a
// method without FSAL in place and takes no unew; zc: the training-form copies za / zs / z7 exist.  An array the method does not have is
// null after Rollout::bind
struct SolveWs { size_t u, un, ut, k[7], za, zs, z7; int s; bool has_un, has_z7, zc; };
SolveWs carve_solve(Arena& a, size_t nb, int s, bool fsal, bool fixed, bool zc) {
    SolveWs w{};
    w.s = s; w.has_un = fsal || !fixed; w.has_z7 = zc && fsal; w.zc = zc;
    w.u = a.take(nb); w.un = a.take(w.has_un ? nb : 0); w.ut = a.take(s > 1 ? nb : 0);
    for (int j = 0; j < 7; ++j) w.k[j] = a.take(j < s ? nb : 0);
    w.za = a.take(zc ? nb : 0); w.zs = a.take(zc && s > 1 ? nb : 0); w.z7 = a.take(w.has_z7 ? nb : 0);
    return w;
}

struct Rollout {
    mgn_engine* h;
    mgn_rollout_desc* d;
    TimeGrid tg;
    int64_t n;                 // rows * O of the state this handle integrates (all N rows, or the owned rows of a partition)
    int64_t n_global = 0;      // N * O
    int32_t nrows = 0;
    float *u, *unew, *utmp, *k[7], *frames, *saves;
    uint8_t* mask;
    double* partial;
    int n_rhs = 0;
    // rows: the rows of the state this handle integrates (all N, or the owned rows of a partition; B N for a pass of B windows)
    Rollout(mgn_engine* h_, mgn_rollout_desc* d_, const TimeGrid& g, bool train_ = false, int32_t rows = 0, int32_t rows_global = 0)
        : h(h_), d(d_), tg(g), n((int64_t)rows * h_->cfg.O), n_global((int64_t)rows_global * h_->cfg.O), nrows(rows) { train = train_; }
    // the solve workspace (carve_solve) at base
    void bind(char* base, const SolveWs& w) {
        auto at = [&](size_t off, bool have) { return have ? (float*)(base + off) : nullptr; };
        u = at(w.u, true); unew = at(w.un, w.has_un); utmp = at(w.ut, w.s > 1);
        for (int j = 0; j < 7; ++j) k[j] = at(w.k[j], j < w.s);
        za = at(w.za, w.zc); zs = at(w.zs, w.zc && w.s > 1); z7 = at(w.z7, w.has_z7);
    }
    double tt(double v) const { return tg.tt(v); }

    // One right-hand side is ~35 launches; on a small mesh they are latency-bound, so each distinct (x, kout) pair of the
    // solver (1 for Euler, 7 for Tsit5) gets its launch sequence captured once and replayed (hipGraph).
    struct RhsGraph { float* x; float* kout; hipGraphExec_t exec; };
    std::vector<RhsGraph> graphs;
    bool warmed = false;

    bool lnall_edges_done = false;
    int rhs_launches(float* x, float* kout) {
        const mgn_config& c = h->cfg;
        if (c.ln_dims == MGN_LN_ALL) {     // the unfused whole-array right-hand side (mgn_train.cpp); its first evaluation encodes the edges
            const int rc = lnall_rhs_dev(h, x, kout, lnall_edges_done);
            lnall_edges_done = true;
            return rc;
        }
        h->srcA_override = x;
        h->out_override = kout;
        int rc = encode_impl(h, true, true, false);
        if (!rc) {
            // encoded edge latents are identical for every RHS of a trajectory (static edge features, frozen e_norm)
            const bool bf = c.dtype == MGN_BF16;
            const size_t eb = tile_floats(h->es[0].ntiles_e, c.L) * (bf ? 2 : 4);
            if (elat_src_ok(h)) {
                h->elat_src_override = reinterpret_cast<const float*>(h->ode.as<char>() + elat0_off);
            } else {
                hipError_t e = hipMemcpyAsync(bf ? h->es[0].bElat.p : h->es[0].Elat.p, h->ode.as<char>() + elat0_off, eb, hipMemcpyDeviceToDevice, h->stream);
                if (e != hipSuccess) rc = fail(h, MGN_E_HIP, "rollout: Elat restore failed: %s", hipGetErrorString(e));
            }
        }
        if (!rc) rc = run_processor(h, c.mps);
        h->elat_src_override = nullptr;
        if (!rc) rc = decode_impl(h, true);
        h->srcA_override = nullptr;
        h->out_override = nullptr;
        return rc;
    }

    // data[field][:, :, floor(Int, t / saves_dt) + 1] (reference src/solve.jl:151): the quotient in the solver's own time type,
    // no tolerance -- a t that sits an ulp below a frame boundary re-uses the previous frame there too -- and an index outside
    // the data is the reference's BoundsError.  MGN_INFLOW_TOLERANT: nearest-below with a guard of 1e-3 frames (a Float32 time drifts by ~1e-4 frames), clamped.
    int frame_index(double t, int64_t* out) const {
        int64_t fr;
        if (d->inflow_rule == MGN_INFLOW_TOLERANT) {
            fr = (int64_t)std::floor(t / tg.sdt + 1e-3);
            if (fr < 0) fr = 0;
            if (fr >= d->n_frames) fr = d->n_frames - 1;
        } else {
            fr = (int64_t)std::floor(tt(t / tg.sdt));
            if (fr < 0 || fr >= d->n_frames)
                return fail(h, MGN_E_ARG, "mgn_rollout: inflow frame %lld at t = %.9g is outside the %d frames given (reference: BoundsError)",
                            (long long)fr, t, d->n_frames);
        }
        *out = fr;
        return MGN_OK;
    }

    // mgn_shooting_grad: the state holds windows of win_rows rows whose frames were chosen on the host, RHS evaluation e of the solve
    // reading ftab[e * ftab_ld + window] (frames [n_frames][win_rows][O], mask [win_rows])
    const int32_t* ftab = nullptr;
    int64_t ftab_ld = 0, win_rows = 0;

    // f(x, t): in-place inflow overwrite of x, then dx/dt -> kout    (ode_func_eval, reference src/solve.jl:147-158)
    // written: x already holds the inflow rows of t's frame (launch_tsit5_stage_input wrote them with the stage sum)
    int rhs(float* x, double t, float* kout, bool written = false) {
        const mgn_config& c = h->cfg;
        const bool overwrite = mask && frames && !written;
        if (overwrite && ftab) {
            HIPCHK(h, launch_shoot_overwrite(x, frames, mask, ftab + (size_t)n_rhs * ftab_ld, win_rows, c.O, nrows, h->stream));
        } else if (overwrite) {
            int64_t fr;
            if (int rc = frame_index(t, &fr)) return rc;
            HIPCHK(h, launch_overwrite(x, frames + (size_t)fr * n, mask, nrows, c.O, h->stream));
        }
        ++n_rhs;
        const bool graphable = h->use_graph && !h->prof && h->stream != nullptr && h->cfg.nranks == 1 && launch_is_small(h->ntiles_n);
        if (!graphable || !warmed) {       // the first RHS runs eagerly: it sets the per-kernel attributes outside of any capture
            warmed = true;
            return rhs_launches(x, kout);
        }
        for (const RhsGraph& g : graphs)
            if (g.x == x && g.kout == kout) {
                HIPCHK(h, hipGraphLaunch(g.exec, h->stream));
                return MGN_OK;
            }
        hipGraphExec_t exec = nullptr;
        const int rc = capture_and_launch(h, h->stream, exec, [&]() -> int { return rhs_launches(x, kout); });
        if (exec) graphs.push_back({x, kout, exec});
        return rc;
    }
    ~Rollout() {
        for (RhsGraph& g : graphs) (void)hipGraphExecDestroy(g.exec);
    }
    size_t elat0_off = 0;

    int norm(const float* a, const float* b, const LinComb& lc, float dt, double* out) {
        const int np_ = errnorm_partials();
        HIPCHK(h, launch_errnorm(a, b, lc, dt, d->abstol, d->reltol, n, partial, h->stream));
        std::vector<double> r(np_);
        HIPCHK(h, hipMemcpyAsync(r.data(), partial, np_ * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        double s = 0;
        for (double v : r) s += v;
        if (h->cfg.nranks != 1) {      // the same bits on every rank -> the same accept / reject decisions
            if (h->comm->allreduce_f64(&s, 1, 0, h->stream) != 0) return fail(h, MGN_E_RCCL, "rollout: error-norm reduction failed: %s", h->comm->err.c_str());
        }
        const int64_t ng = n_global > 0 ? n_global : n;
        *out = std::sqrt(s / (double)(ng > 0 ? ng : 1));
        return MGN_OK;
    }

    // ---- saves ----
    int saved = 0;                         // saves taken
    std::vector<int64_t> save_step;        // the accepted steps before each save taken
    // dense saves (mgn_solver_grad_tsit5 with MGN_TSIT5_DENSE_SAVES): the only stop is t1, and a save no step ends on is interpolated
    // inside the accepted step that passes it -- save_step its index, save_theta where (< 0: the save is the state after save_step steps)
    bool dense = false;
    std::vector<double> save_theta;
    // mgn_rollout_eval: every save is compared with its ground-truth frame as it is produced (k_save_error) -- gt [n_saves][n] in the
    // engine's order, acc [n] doubles, part [n_saves][save_error_blocks(nrows)][O] -- and kept only if the caller wants the solution
    const float* ev_gt = nullptr;
    double *ev_acc = nullptr, *ev_part = nullptr;
    // mgn_rollout_eval: save number `saved`, held in x, against its ground-truth frame
    int save_error(const float* x) {
        if (ev_gt)
            HIPCHK(h, launch_save_error(x, ev_gt + (size_t)saved * n, ev_acc, ev_part + (size_t)saved * save_error_blocks(nrows) * h->cfg.O, nrows,
                                        h->cfg.O, h->stream));
        return MGN_OK;
    }
    // saves[saved] <- u, the state after steps_done accepted steps
    int save(int64_t steps_done) {
        save_step.push_back(steps_done);
        save_theta.push_back(-1.0);
        if (int rc = save_error(u)) return rc;
        if (saves) HIPCHK(h, hipMemcpyAsync(saves + (size_t)saved * n, u, (size_t)n * 4, hipMemcpyDeviceToDevice, h->stream));
        ++saved;
        return MGN_OK;
    }
    // does pending save time ts sit on a step's end tn?  (at most tn, and within the tolerance the stops are hit with)
    static bool hits(double ts, double tn) { return ts <= tn && std::fabs(ts - tn) <= 1e-9 * std::fabs(tn) + 1e-12; }
    // dense saves: the pending saves strictly inside the accepted trial of step nstep from t to tn with size hstep, before erk_advance
    // (u = x_n, k[0 .. 6] = k_{n,1 .. 7}): saves[saved] <- x_n + hstep sum_i b_i(theta) k_{n,i}, theta = (ts - t) / hstep formed in double
    // from the time-type values (at most 1: tn is rounded), the weights rounded to float once.  The interpolant is formed once, in the save's
    // slot or -- mgn_rollout_eval without d->out -- in utmp (the stage-6 input, free once k6 exists), and reduced from there as save()
    // reduces the state: the error outputs are the same bits with and without a solution buffer
    int saves_inside(int64_t nstep, double t, double hstep, double tn) {
        while (saved < d->n_saves) {
            const double ts = tg.stop_time(saved);
            if (ts > tn || hits(ts, tn)) break;
            const double theta = std::min((ts - t) / hstep, 1.0);
            double b[7];
            if (mgn_tsit5_interp_weights(theta, b) != MGN_OK) return fail(h, MGN_E_STATE, "dense save %d: theta = %g", saved, theta);
            LinComb lc{7, {}, {}};
            for (int j = 0; j < 7; ++j) { lc.c[j] = (float)b[j]; lc.k[j] = k[j]; }
            float* xs = saves ? saves + (size_t)saved * n : utmp;
            HIPCHK(h, launch_lincomb(xs, u, lc, (float)hstep, n, h->stream));
            if (int rc = save_error(xs)) return rc;
            save_step.push_back(nstep);
            save_theta.push_back(theta);
            ++saved;
        }
        return MGN_OK;
    }
    // ... and, after the advance to t (nacc steps done), the save that sits on it
    int saves_on(int64_t nacc, double t) {
        while (saved < d->n_saves && hits(tg.stop_time(saved), t))
            if (int rc = save(nacc)) return rc;
        return MGN_OK;
    }
    // the saves a fixed-step plan (the accepted steps before every save, fixed_grid) takes after steps_done steps
    int saves_after(const std::vector<int64_t>& plan, int64_t steps_done) {
        while (saved < (int)plan.size() && plan[saved] == steps_done)
            if (int rc = save(steps_done)) return rc;
        return MGN_OK;
    }

    // Training form (solver-based training, ode_func_train): the right-hand side sees a COPY of its input with the inflow rows written --
    // za for stage 1 (z_{n,1}), zs for stages 2 .. s', z7 for the FSAL stage (Tsit5's stage 7, z_{n+1,1}) -- and the state is never
    // overwritten.  mgn_rollout (train = false), or no inflow mask: the input itself (mgn_rollout overwrites it in place).
    bool train = false;
    float *za = nullptr, *zs = nullptr, *z7 = nullptr;
    float* kept = nullptr;     // training form: the current trial's stage inputs [s'][n] (z_{n,1}, stages 2 .. s'), or null

    // the array the right-hand side of input y sees (z: its training-form copy)
    float* rhs_input(float* y, float* z) const { return (train && mask) ? z : y; }
    int eval(float* y, float* z, double t, float* kout) {
        float* x = rhs_input(y, z);
        if (x != y) HIPCHK(h, hipMemcpyAsync(x, y, (size_t)n * 4, hipMemcpyDeviceToDevice, h->stream));
        return rhs(x, t, kout);
    }

    // ---- fixed-step Euler as mgn_rollout runs it: the inflow rows written into the state itself, a save on every save point reached ----
    int euler_rollout() {
        if (int rc = save(0)) return rc;   // solution at t0
        double t = tg.t0;
        const int64_t nsteps = (int64_t)std::llround((tg.t1 - tg.t0) / tg.dt);
        for (int64_t i = 0; i < nsteps; ++i) {
            if (int rc = rhs(u, t, k[0])) return rc;
            LinComb lc{1, {1.f}, {k[0]}};
            HIPCHK(h, launch_lincomb(u, u, lc, (float)tg.dt, n, h->stream));
            t = tg.next(i, nsteps, t);
            ++d->n_accept;
            // saveat: the state of the step that ends at the save point.  In its own time type the integrator's t drifts off the
            // save grid by a few ulps per step (Float32: ~1e-6 s after 600 steps of 0.01 s); the reference interpolates there, which
            // moves the saved state by (drift / dt) of one step's change -- far below the rollout tolerance -- so: the nearest step.
            while (saved < d->n_saves && tg.stop_time(saved) <= t + 0.25 * tg.dt)
                if (int rc = save(i + 1)) return rc;
        }
        while (saved < d->n_saves)      // (t1 short of the last stop: repeat the final state)
            if (int rc = save(nsteps)) return rc;
        return MGN_OK;
    }

    // ---- explicit Runge-Kutta by tableau (tb: Tsit5's unless mgn_rollout_erk gave another), shared by mgn_rollout, mgn_rollout_erk,
    // mgn_solver_grad_tsit5 and mgn_shooting_grad ----
    const Erk* tb = &erk_tsit5();
    bool have_k1 = false;      // k[0] = f(u): kept over the retrials of a step; FSAL keeps it over accepted steps too
    // k1 = f(u) at t (FSAL afterwards)
    int erk_first(double t) {
        have_k1 = true;
        return eval(u, za, t, k[0]);
    }
    // sum over the stages j < m of coef[j] k_j, coefficients rounded to float once, terms whose coefficient is exactly 0 left out
    LinComb stage_sum(const double* coef, int m) const {
        LinComb lc{0, {}, {}};
        for (int j = 0; j < m; ++j)
            if (coef[j] != 0.0) { lc.c[lc.n] = (float)coef[j]; lc.k[lc.n] = k[j]; ++lc.n; }
        return lc;
    }
    // Hairer-Wanner starting step from (u, k1)
    int erk_h0(double t, double* dt) {
        double d0, d1, d2;
        LinComb l1{1, {1.f}, {k[0]}};
        // d0 = ||u||, d1 = ||f0|| in the scaled norm: errnorm(dt = 1) of u and k1 themselves
        LinComb lu{1, {1.f}, {u}};
        if (int rc = norm(u, u, lu, 1.f, &d0)) return rc;
        if (int rc = norm(u, u, l1, 1.f, &d1)) return rc;
        const double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
        HIPCHK(h, launch_lincomb(utmp, u, l1, (float)h0, n, h->stream));
        if (int rc = eval(utmp, zs, tt(t + h0), k[1])) return rc;
        LinComb ld{2, {1.f, -1.f}, {k[1], k[0]}};
        if (int rc = norm(u, u, ld, (float)(1.0 / h0), &d2)) return rc;
        const double mx = d1 > d2 ? d1 : d2;
        const double h1 = mx <= 1e-15 ? (h0 * 1e-3 > 1e-6 ? h0 * 1e-3 : 1e-6) : std::pow(0.01 / mx, 1.0 / tb->p);
        *dt = 100 * h0 < h1 ? 100 * h0 : h1;
        return MGN_OK;
    }
    // one trial step from (u, k1) over hstep: stages 2 .. s at tt(t + tt(c_i hstep)) on utmp; the FSAL stage (stage s of an FSAL tableau:
    // Tsit5's k7) is f(unew), unew = u + hstep sum_j b_j k_j, at t7; without FSAL unew is formed after the last stage and not evaluated.
    // EEst (null: none, the fixed-step mode) the scaled error norm of the embedded pair -- one small D2H.
    // in_place (erk_fixed, without FSAL): the new state is formed in u itself -- no trial is rejected there, the stage inputs live in utmp,
    // and the right-hand side keeps one input array from step to step (one captured graph per stage, not two)
    // fused_input (the fixed-step loops of mgn_rollout and mgn_rollout_erk): the stage sum and the in-place inflow rows of its stage time
    // in one launch (launch_tsit5_stage_input: launch_lincomb's bits, then launch_overwrite's rows) where the other loops issue two
    bool fused_input = false, in_place = false;
    int erk_trial(double t, double hstep, double t7, double* EEst) {
        const Erk& e = *tb;
        const int last = e.s - 1, active = e.s - (e.fsal ? 1 : 0);      // active: the stages whose inputs the training form keeps
        for (int sidx = 1; sidx < e.s; ++sidx) {     // stages 2..s
            const bool on_new = e.fsal && sidx == last;
            const LinComb lc = stage_sum(e.A[sidx], sidx);
            float* dst = on_new ? unew : utmp;
            const double ts = on_new ? t7 : tt(t + tt(e.c[sidx] * hstep));
            if (fused_input) {
                const float* fr = nullptr;
                if (mask && frames) {
                    int64_t f;
                    if (int rc = frame_index(ts, &f)) return rc;
                    fr = frames + (size_t)f * n;
                }
                HIPCHK(h, launch_tsit5_stage_input(dst, u, lc, (float)hstep, fr, fr ? mask : nullptr, nrows, h->cfg.O, h->stream));
                if (int rc = rhs(dst, ts, k[sidx], true)) return rc;
                continue;
            }
            HIPCHK(h, launch_lincomb(dst, u, lc, (float)hstep, n, h->stream));
            float* z = on_new ? z7 : zs;
            if (int rc = eval(dst, z, ts, k[sidx])) return rc;
            if (sidx < active && kept)
                HIPCHK(h, hipMemcpyAsync(kept + (size_t)sidx * n, rhs_input(dst, z), (size_t)n * 4, hipMemcpyDeviceToDevice, h->stream));
        }
        if (!e.fsal) HIPCHK(h, launch_lincomb(in_place ? u : unew, u, stage_sum(e.b, e.s), (float)hstep, n, h->stream));
        if (!EEst) return MGN_OK;
        return norm(u, unew, stage_sum(e.bt, e.s), (float)hstep, EEst);
    }
    // the accepted trial becomes the state: unew -> u (in_place: it is there); FSAL: the last stage -> k1 (Tsit5: k7), z_{n+1,1} -> za;
    // otherwise k1 is due again
    void erk_advance() {
        if (!in_place) std::swap(u, unew);
        if (tb->fsal) {
            std::swap(k[0], k[tb->s - 1]);
            std::swap(za, z7);
        } else {
            have_k1 = false;
        }
    }

    // training form: slot(n, &p) gives accepted step n's storage for its s' stage inputs
    using Slot = std::function<int(int64_t, float**)>;
    std::vector<double> step_t, step_h;    // training form: every accepted step's t and h
    // before a trial of step n: its storage, and z_{n,1} (what k1's right-hand side saw) into it
    int begin_trial(const Slot& slot, int64_t n_) {
        if (int rc = slot(n_, &kept)) return rc;
        HIPCHK(h, hipMemcpyAsync(kept, rhs_input(u, za), (size_t)n * 4, hipMemcpyDeviceToDevice, h->stream));
        return MGN_OK;
    }

    // fixed steps of the tableau: K steps of dt on the fixed grid, the FSAL stage at t_{n+1}; saves from the plan.  slot: the training
    // form (mgn_solver_grad_tsit5, mgn_solver_grad_erk, mgn_shooting_grad), every step's stage inputs and record kept; none: the
    // evaluation form of mgn_rollout_erk, nothing stored
    int erk_fixed(int64_t K, const std::vector<int64_t>& plan, const Slot* slot) {
        double t = tg.t0;
        in_place = !tb->fsal;
        if (int rc = saves_after(plan, 0)) return rc;
        if (tb->fsal)
            if (int rc = erk_first(t)) return rc;
        for (int64_t i = 0; i < K; ++i) {
            const double tn = tg.next(i, K, t);
            if (!have_k1)
                if (int rc = erk_first(t)) return rc;
            if (slot)
                if (int rc = begin_trial(*slot, i)) return rc;
            if (int rc = erk_trial(t, tg.dt, tn, nullptr)) return rc;
            erk_advance();
            if (slot) { step_t.push_back(t); step_h.push_back(tg.dt); }
            t = tn;
            ++d->n_accept;
            if (int rc = saves_after(plan, i + 1)) return rc;
        }
        kept = nullptr;
        return MGN_OK;
    }

    // fixed steps with dense saves, solve(...; adaptive = false, dt, saveat = saves): t <- tt(t + dt) with h = dt until t1; a step whose
    // end lies within 1e-5 saves_dt of t1 snaps onto it (TimeGrid::next's rule), one that would pass t1 is cut to h = tt(t1 - t).  dt
    // need not divide saves_dt; the saves are interpolated (saves_inside) or sit on a step's end.  One loop for mode 2 of
    // mgn_solver_grad_tsit5 (slot: the training form, every step's stage inputs and record kept) and solver MGN_SOLVER_TSIT5_FIXED of
    // mgn_rollout (no slot: the evaluation form, nothing stored)
    int tsit5_fixed_dense(const Slot* slot) {
        double t = tg.t0;
        if (int rc = save(0)) return rc;
        if (int rc = erk_first(t)) return rc;
        int64_t nacc = 0;
        while (t < tg.t1 - 1e-5 * tg.sdt) {
            double hstep = tg.dt, tn = tt(t + tg.dt);
            if (std::fabs(tn - tg.t1) <= 1e-5 * tg.sdt) tn = tg.t1;
            else if (tn > tg.t1) { hstep = tt(tg.t1 - t); tn = tg.t1; }
            if (slot)
                if (int rc = begin_trial(*slot, nacc)) return rc;
            if (int rc = erk_trial(t, hstep, tn, nullptr)) return rc;
            if (int rc = saves_inside(nacc, t, hstep, tn)) return rc;
            erk_advance();
            if (slot) { step_t.push_back(t); step_h.push_back(hstep); }
            t = tn;
            ++nacc;
            ++d->n_accept;
            if (int rc = saves_on(nacc, t)) return rc;
        }
        kept = nullptr;
        while (saved < d->n_saves)      // (saves the solve stops an ulp short of: the final state)
            if (int rc = save(nacc)) return rc;
        return MGN_OK;
    }

    // adaptive Tsit5 from t0 to t1: mgn_rollout's PI controller (StepControl), tstops = saves, a save on every stop it hits, missing saves
    // (t1 short of the last stop) padded with the final state.  mgn_rollout (no slot): stage 7 at c7 h, and the iteration guard stops
    // silently.  Training form (slot): every trial's stage inputs kept in slot(n), stage 7 is z_{n+1,1} and sees t_{n+1}, the accepted
    // steps recorded, and the guard fails the call.  dense (training form only): no stop but t1, the saves as tsit5_fixed_dense takes them.
    int erk_adaptive(const char* who, const Slot* slot) {
        const int ns = d->n_saves;
        double t = tg.t0;
        if (int rc = save(0)) return rc;
        double dt = tg.dt;
        if (tb->fsal || dt <= 0)
            if (int rc = erk_first(t)) return rc;     // k1 (FSAL afterwards; otherwise once per state that starts a step, below)
        if (dt <= 0)   // Hairer-Wanner starting step
            if (int rc = erk_h0(t, &dt)) return rc;
        StepControl ctl(*tb);
        int64_t guard = 0, nacc = 0;
        // float32 descriptors: t1 and n*saves_dt may differ in the last ulp; an interval shorter than 1e-5 save periods is not worth a step
        while (t < tg.t1 - 1e-5 * tg.sdt) {
            if (++guard >= 10000000) {
                if (!slot) break;
                return fail(h, MGN_E_STATE, "%s: %lld trial steps without reaching t1", who, (long long)guard);
            }
            double tstop = (saved < ns && !dense) ? tg.stop_time(saved) : tg.t1;
            if (tstop > tg.t1) tstop = tg.t1;
            bool hit_stop = false;
            double hstep = dt;
            if (t + hstep >= tstop - 1e-9 * std::fabs(tstop)) { hstep = tstop - t; hit_stop = true; }
            const double tn = hit_stop ? tstop : tt(t + hstep);
            // (a stage that lands on the stop itself sees the stop's time: c7 = 1)
            const double t7 = (slot || hit_stop) ? tn : tt(t + tt(tb->c[tb->s - 1] * hstep));
            if (!have_k1)
                if (int rc = erk_first(t)) return rc;
            if (slot)
                if (int rc = begin_trial(*slot, nacc)) return rc;
            double EEst;
            if (int rc = erk_trial(t, hstep, t7, &EEst)) return rc;
            if (!(EEst == EEst)) return fail(h, MGN_E_STATE, "%s: NaN in the error estimate at t = %g", who, t);
            if (ctl.decide(EEst, hstep, hit_stop, dt)) {
                if (dense)
                    if (int rc = saves_inside(nacc, t, hstep, tn)) return rc;
                erk_advance();
                if (slot) { step_t.push_back(t); step_h.push_back(hstep); }
                t = tn;
                ++nacc;
                ++d->n_accept;
                if (dense) {
                    if (int rc = saves_on(nacc, t)) return rc;
                } else if (hit_stop && saved < ns && std::fabs(tg.stop_time(saved) - t) <= 1e-9 * std::fabs(t) + 1e-12) {
                    if (int rc = save(nacc)) return rc;
                }
            } else {
                ++d->n_reject;
            }
        }
        kept = nullptr;
        while (saved < ns)
            if (int rc = save(nacc)) return rc;
        return MGN_OK;
    }
};
// b.ensure(bytes), or MGN_E_OOM (MGN_E_HIP for any other error) with the message "<what>: <the HIP error>"
__attribute__((format(printf, 4, 5))) int ensure_or_fail(mgn_handle* h, DevBuf& b, size_t bytes, const char* what, ...) {
    const hipError_t e = b.ensure(bytes);
    if (e == hipSuccess) return MGN_OK;
    (void)hipGetLastError();
    char msg[400];
    va_list ap;
    va_start(ap, what);
    vsnprintf(msg, sizeof msg, what, ap);
    va_end(ap);
    return fail(h, e == hipErrorOutOfMemory ? MGN_E_OOM : MGN_E_HIP, "%s: %s", msg, hipGetErrorString(e));
}

// x0 (u null: not wanted), the inflow frames and the inflow mask (null: none) of the caller's order into the engine's order on the device:
// the rows this handle owns (all N, or a partition's), renumbered or not.  A reordered copy is staged on the host and synchronised.
int upload_engine_order(mgn_handle* h, const mgn_rollout_desc* d, float* u, float* frames, uint8_t* mask) {
    const LocalGraph& g = h->g;
    const int O = h->cfg.O;
    const bool part = h->cfg.nranks != 1;
    const int32_t nloc = part ? g.n_own : g.N;
    const int nf = frames ? d->n_frames : 0;
    const size_t nb = (size_t)nloc * O * 4, fb = (size_t)nf * nb;
    if (!part && !g.renumbered) {
        if (u) HIPCHK(h, hipMemcpyAsync(u, d->x0, nb, hipMemcpyHostToDevice, h->stream));
        if (frames) HIPCHK(h, hipMemcpyAsync(frames, d->inflow_data, fb, hipMemcpyHostToDevice, h->stream));
        if (mask) HIPCHK(h, hipMemcpyAsync(mask, d->inflow_mask, (size_t)nloc, hipMemcpyHostToDevice, h->stream));
        return MGN_OK;
    }
    std::vector<float> lx((size_t)nloc * O * (1 + nf));
    std::vector<uint8_t> lm(mask ? (size_t)nloc : 0);
    for (int32_t i = 0; i < nloc; ++i) {
        const size_t gi = (size_t)g.own_gid[i];
        if (u) memcpy(lx.data() + (size_t)i * O, d->x0 + gi * O, (size_t)O * 4);
        for (int f = 0; f < nf; ++f)
            memcpy(lx.data() + ((size_t)(1 + f) * nloc + i) * O, d->inflow_data + ((size_t)f * g.N + gi) * O, (size_t)O * 4);
        if (mask) lm[i] = d->inflow_mask[gi];
    }
    if (u) HIPCHK(h, hipMemcpyAsync(u, lx.data(), nb, hipMemcpyHostToDevice, h->stream));
    if (frames) HIPCHK(h, hipMemcpyAsync(frames, lx.data() + (size_t)nloc * O, fb, hipMemcpyHostToDevice, h->stream));
    if (mask) HIPCHK(h, hipMemcpyAsync(mask, lm.data(), (size_t)nloc, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return MGN_OK;
}

// count [N][O] arrays in the engine's order on the device (one partition) into the caller's order on the host; the caller synchronises
int saves_to_caller(mgn_handle* h, const float* src, int64_t count, float* out) {
    const LocalGraph& g = h->g;
    const int O = h->cfg.O;
    const size_t bytes = (size_t)count * g.N * O * 4;
    if (!g.renumbered) {
        HIPCHK(h, hipMemcpyAsync(out, src, bytes, hipMemcpyDeviceToHost, h->stream));
        return MGN_OK;
    }
    std::vector<float> sv((size_t)count * g.N * O);
    HIPCHK(h, hipMemcpyAsync(sv.data(), src, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int64_t i = 0; i < count; ++i)
        for (int32_t j = 0; j < g.N; ++j)
            memcpy(out + ((size_t)i * g.N + (size_t)g.own_gid[j]) * O, sv.data() + ((size_t)i * g.N + j) * O, (size_t)O * 4);
    return MGN_OK;
}

// the static inputs of a solve (one-hot node types, raw edge features, val_mask; x0 only fills the encoder's state slot: every right-hand
// side reads its state through srcA_override), and the edges encoded ONCE per trajectory into elat0 (eb: its fp32 bytes)
int upload_statics(mgn_handle* h, const mgn_rollout_desc* d, const float* x0, char* elat0, size_t eb) {
    const mgn_config& c = h->cfg;
    if (int rc = upload_inputs(h, x0, c.O, d->node_type_onehot, c.Fn - c.O, d->ef_raw, true)) return rc;
    h->have_mask = d->val_mask != nullptr;
    if (d->val_mask) {
        HIPCHK(h, h->d_mask.ensure((size_t)h->g.N * 4));
        HIPCHK(h, hipMemcpyAsync(h->d_mask.p, d->val_mask, (size_t)h->g.N * 4, hipMemcpyHostToDevice, h->stream));
    }
    if (c.ln_dims == MGN_LN_ALL) return lnall_rhs_prepare(h);
    if (int rc = encode_impl(h, true, false, true)) return rc;
    const bool bf = is_bf16(h);
    HIPCHK(h, hipMemcpyAsync(elat0, bf ? h->es[0].bElat.p : h->es[0].Elat.p, bf ? eb / 2 : eb, hipMemcpyDeviceToDevice, h->stream));
    return MGN_OK;
}

// the handle's state that solver-based training needs: a device handle, one partition, fp32, one edge set, parameters and a graph
int solver_state_checks(mgn_handle* h, const char* who, bool partitions = false) {
    if (int rc = width_refuse(h, who)) return rc;
    if (h->host_only) return fail(h, MGN_E_HIP, "host-only handle (MGN_DEVICE_NONE): no compute path; create the handle on a HIP device");
    const mgn_config& c = h->cfg;
    if (c.nranks != 1 && !partitions) return fail(h, MGN_E_STATE, "%s drives one partition", who);
    if (c.dtype != MGN_F32) return fail(h, MGN_E_STATE, "%s computes in fp32: create the handle with dtype MGN_F32", who);
    if (h->nsets != 1) return fail(h, MGN_E_STATE, "%s mirrors the reference's single-edge-set RHS (src/solve.jl:188-219); this handle has two edge sets", who);
    return need(h, true, true, c.ln_dims != MGN_LN_ALL, true);
}

// the static inputs of the right-hand side
int solver_static_checks(mgn_handle* h, const mgn_rollout_desc* d, const char* who) {
    const mgn_config& c = h->cfg;
    if (!d->ef_raw || (c.Fn > c.O && !d->node_type_onehot)) return fail(h, MGN_E_ARG, "%s: null argument", who);
    if (c.Fn < c.O) return fail(h, MGN_E_ARG, "%s: Fn < O", who);
    return MGN_OK;
}

// the inflow rule and its arrays
int inflow_checks(mgn_handle* h, const mgn_rollout_desc* d, const char* who) {
    if (d->inflow_rule != MGN_INFLOW_REFERENCE && d->inflow_rule != MGN_INFLOW_TOLERANT) return fail(h, MGN_E_ARG, "%s: unknown inflow_rule", who);
    if ((d->inflow_mask != nullptr) != (d->inflow_data != nullptr)) return fail(h, MGN_E_ARG, "%s: inflow mask and data go together", who);
    return MGN_OK;
}

// count [N][O] arrays (host or device, the caller's order) into the engine's order at dst, gathered on the device through tmp ([N][O] scratch)
// when the graph is renumbered.  A partition keeps the rows it owns of every array: dst is [count][n_own][O], tmp still [N][O]
int to_engine_order(mgn_handle* h, const float* src, int64_t count, float* dst, float* tmp) {
    const int32_t N = h->g.N;
    const int O = h->cfg.O;
    const size_t n = (size_t)N * O;
    if (h->cfg.nranks != 1) {
        const size_t nl = (size_t)h->g.n_own * O;
        for (int64_t s = 0; s < count; ++s) {
            HIPCHK(h, hipMemcpyAsync(tmp, src + s * n, n * 4, hipMemcpyDefault, h->stream));
            HIPCHK(h, launch_permute_rows(dst + s * nl, tmp, h->d_own_gid.as<int32_t>(), h->g.n_own, O, false, h->stream));
        }
        return MGN_OK;
    }
    for (int64_t s = 0; s < count; ++s) {
        HIPCHK(h, hipMemcpyAsync(h->g.renumbered ? tmp : dst + s * n, src + s * n, n * 4, hipMemcpyDefault, h->stream));
        if (h->g.renumbered) HIPCHK(h, launch_permute_rows(dst + s * n, tmp, h->d_own_gid.as<int32_t>(), N, O, false, h->stream));
    }
    return MGN_OK;
}

// mgn_rollout (e null) and mgn_rollout_eval (e: its checked descriptor): the same solve, the same launches in the same order; with e
// every save is reduced against its ground-truth frame as it is produced (Rollout::save) and d->out is optional.
// e on a partitioned mesh (mgn_group_rollout_eval): every rank reduces the rows it owns -- sel's entries whose node it owns, mapped to
// its rows, as often as they are listed --, then the ranks' sums ([n_saves][O] per-save sums and the val_loss numerator, undivided) are
// folded once in ascending rank order (rank_fold_f64) and divided by the whole mesh's counts; mse_time's rows go through
// gather_rows_global.  Without d->out no save is kept, gathered or downloaded on any rank.
// tab (mgn_rollout_erk and its kin; null: the solver d->solver names): the method is this tableau, already checked, d->solver is not read,
// and adaptive chooses between the fixed grid (Rollout::erk_fixed without a slot) and the controller's loop (Rollout::erk_adaptive)
int fixed_grid(mgn_handle* h, const char* who, const TimeGrid& T, int n_saves, int64_t* K, std::vector<int64_t>& save_step);
int rollout_solve(mgn_handle* h, mgn_rollout_desc* d, mgn_rollout_eval_desc* e, const char* who, const double* tab = nullptr, int32_t adaptive = 0) {
    const bool lnall = h && h->cfg.ln_dims == MGN_LN_ALL;
    if (int rc = need(h, true, true, !lnall, true)) return rc;
    if (tab) {
        if (!d) return fail(h, MGN_E_ARG, "%s: null argument", who);
        if (adaptive != 0 && adaptive != 1) return fail(h, MGN_E_ARG, "%s: adaptive must be 0 or 1", who);
        if (adaptive && tab[3] == 0.0)
            return fail(h, MGN_E_UNSUPPORTED, "%s: adaptive = 1 needs a tableau with an embedded pair (btilde); this one has none", who);
    }
    const mgn_config& c = h->cfg;
    const bool part = c.nranks != 1;      // partitioned: every rank integrates the rows it owns; error norms are reduced over the ranks
    if (part) if (int rc = need_comm(h, who)) return rc;
    if (h->nsets != 1) return fail(h, MGN_E_STATE, "%s mirrors the reference's single-edge-set RHS (src/solve.jl:188-219); this handle has two edge sets", who);
    if (!d || !d->x0 || (!d->out && !e)) return fail(h, MGN_E_ARG, "%s: null argument", who);
    if (int rc = solver_static_checks(h, d, who)) return rc;
    const TimeGrid T(d);
    if (d->n_saves < 1 || !(T.sdt > 0.0) || T.t1 < T.t0) return fail(h, MGN_E_ARG, "%s: bad time grid", who);
    int64_t erk_K = 0;                      // a tableau with fixed steps: the step count and the accepted steps before every save
    std::vector<int64_t> erk_plan;
    if (tab) {
        if (!adaptive) {
            if (!(T.dt > 0.0)) return fail(h, MGN_E_ARG, "%s: fixed steps need dt > 0", who);
            const double per = T.sdt / T.dt, m = std::round(per);
            if (!(m >= 1.0) || std::fabs(per - m) > 1e-6 * m)
                return fail(h, MGN_E_ARG, "%s: saves_dt / dt = %.9g is not an integer >= 1: a general tableau has no dense output (Tsit5 with other "
                            "steps: mgn_rollout with MGN_SOLVER_TSIT5_FIXED)", who, per);
            if (int rc = fixed_grid(h, who, T, d->n_saves, &erk_K, erk_plan)) return rc;
        } else if (d->abstol <= 0.f || d->reltol <= 0.f) {
            return fail(h, MGN_E_ARG, "%s: tolerances must be > 0", who);
        }
        if (int rc = inflow_checks(h, d, who)) return rc;
    } else {
        if (d->solver == MGN_SOLVER_EULER && !(T.dt > 0.0)) return fail(h, MGN_E_ARG, "%s: Euler needs dt > 0", who);
        if (d->solver == MGN_SOLVER_TSIT5_FIXED && !(T.dt > 0.0)) return fail(h, MGN_E_ARG, "%s: fixed steps need dt > 0", who);
        if (int rc = inflow_checks(h, d, who)) return rc;
        if (d->solver < MGN_SOLVER_EULER || d->solver > MGN_SOLVER_TSIT5_FIXED)
            return fail(h, MGN_E_ARG, "%s: solver must be 0 (Euler), 1 (Tsit5) or 2 (Tsit5 with fixed steps)", who);
        if (d->solver == MGN_SOLVER_TSIT5 && (d->abstol <= 0.f || d->reltol <= 0.f)) return fail(h, MGN_E_ARG, "%s: tolerances must be > 0", who);
    }
    const LocalGraph& g = h->g;
    invalidate_static(h);
    const int32_t nloc = part ? g.n_own : g.N;        // rows of the state this handle integrates
    Rollout R(h, d, T, false, nloc, g.N);
    const size_t nb = (size_t)R.n * 4;
    const size_t fb = d->inflow_data ? (size_t)d->n_frames * nb : 0, sb = d->out ? (size_t)d->n_saves * nb : 0;
    const size_t eb = tile_floats(h->es[0].ntiles_e, c.L) * 4;
    // evaluation: ground truth that IS the inflow data is compared where upload_engine_order puts the frames; the selection in the
    // engine's order (n_sel == 0: all elements, no index array)
    const bool gt_is_frames = e && e->gt == d->inflow_data && d->n_frames >= d->n_saves;
    const int eblk = e ? save_error_blocks(nloc) : 0;
    int64_t n_val = e ? (e->n_sel > 0 ? e->n_sel : R.n) : 0;      // the elements this handle sums (a partition: those it owns)
    const int64_t n_val_all = e ? (e->n_sel > 0 ? e->n_sel : R.n_global) : 0;   // the divisor: the whole mesh's
    std::vector<int64_t> sel;
    if (e && e->n_sel > 0 && part) {
        std::vector<int32_t> g2l((size_t)g.N, -1);
        for (int32_t i = 0; i < g.n_own; ++i) g2l[(size_t)g.own_gid[i]] = i;
        for (int64_t i = 0; i < e->n_sel; ++i) {
            const int64_t li = (int64_t)e->sel[i] - e->sel_index_base;      // (checked by rollout_eval_run)
            const int32_t l = g2l[(size_t)(li / c.O)];
            if (l >= 0) sel.push_back((int64_t)l * c.O + li % c.O);
        }
        n_val = (int64_t)sel.size();       // (0: this rank owns none of sel and still takes part in every exchange)
    } else if (e && e->n_sel > 0) {
        std::vector<int32_t> g2l;
        if (g.renumbered) {
            g2l.resize((size_t)g.N);
            for (int32_t i = 0; i < g.N; ++i) g2l[(size_t)g.own_gid[i]] = i;
        }
        sel.resize((size_t)e->n_sel);
        for (int64_t i = 0; i < e->n_sel; ++i) {
            const int64_t li = (int64_t)e->sel[i] - e->sel_index_base;      // (checked by mgn_rollout_eval)
            sel[(size_t)i] = g.renumbered ? (int64_t)g2l[(size_t)(li / c.O)] * c.O + li % c.O : li;
        }
    }
    Arena a;
    const SolveWs ws = carve_solve(a, nb, 7, true, false, false);      // (every solver takes Tsit5's arrays: Euler too keeps all seven k and unew)
    const size_t o_fr = a.take(fb), o_sv = a.take(sb), o_mask = a.take((size_t)nloc), o_part = a.take(errnorm_partials() * sizeof(double));
    R.elat0_off = a.take(eb);
    const size_t o_eacc = a.take(e ? (size_t)R.n * 8 : 0), o_epart = a.take((size_t)d->n_saves * eblk * c.O * 8),
                 o_egt = a.take(e && !gt_is_frames ? (size_t)d->n_saves * nb : 0),
                 o_etmp = a.take(e && !gt_is_frames && (g.renumbered || part) ? (size_t)g.N * c.O * 4 : 0),
                 o_esel = a.take(sel.size() * 8), o_evp = a.take(e ? (size_t)save_error_blocks(n_val) * 8 : 0),
                 o_ems = a.take(e && e->mse_save ? (size_t)d->n_saves * c.O * 8 : 0), o_emt = a.take(e && e->mse_time ? nb : 0);
    HIPCHK(h, h->ode.ensure(a.off));
    char* base = h->ode.as<char>();
    R.bind(base, ws);
    R.frames = d->inflow_data ? (float*)(base + o_fr) : nullptr;
    R.saves = d->out ? (float*)(base + o_sv) : nullptr;
    R.mask = d->inflow_mask ? (uint8_t*)(base + o_mask) : nullptr;
    R.partial = (double*)(base + o_part);
    if (int rc = upload_engine_order(h, d, R.u, R.frames, R.mask)) return rc;
    if (int rc = upload_statics(h, d, d->x0, base + R.elat0_off, eb)) return rc;
    if (e) {
        float* gtl = (float*)(base + o_egt);
        if (!gt_is_frames)      // (as solver_targets)
            if (int rc = to_engine_order(h, e->gt, d->n_saves, gtl, (float*)(base + o_etmp))) return rc;
        if (!sel.empty()) HIPCHK(h, hipMemcpyAsync(base + o_esel, sel.data(), sel.size() * 8, hipMemcpyHostToDevice, h->stream));
        R.ev_gt = gt_is_frames ? R.frames : gtl;
        R.ev_acc = (double*)(base + o_eacc);
        R.ev_part = (double*)(base + o_epart);
        HIPCHK(h, hipMemsetAsync(R.ev_acc, 0, (size_t)R.n * 8, h->stream));
    }

    d->n_accept = d->n_reject = 0;
    Erk erk;
    if (tab) {
        erk = erk_unpack(tab);
        R.tb = &erk;
        R.fused_input = !adaptive;
        if (int rc = adaptive ? R.erk_adaptive(who, nullptr) : R.erk_fixed(erk_K, erk_plan, nullptr)) return rc;
    } else {
        R.fused_input = d->solver == MGN_SOLVER_TSIT5_FIXED;
        if (int rc = d->solver == MGN_SOLVER_EULER ? R.euler_rollout() : d->solver == MGN_SOLVER_TSIT5 ? R.erk_adaptive(who, nullptr) : R.tsit5_fixed_dense(nullptr))
            return rc;
    }
    if (part) {     // every rank returns the complete solution (mgn_rollout_eval without d->out: none is kept)
        for (int i = 0; d->out && i < d->n_saves; ++i)
            if (int rc = gather_rows_global(h, R.saves + (size_t)i * R.n, c.O, d->out + (size_t)i * g.N * c.O)) return rc;
    } else if (d->out) {
        if (int rc = saves_to_caller(h, R.saves, d->n_saves, d->out)) return rc;
    }
    std::vector<double> vpart;
    if (e) {
        EvalFinish f{};
        f.acc = R.ev_acc; f.part = R.ev_part; f.N = nloc; f.O = c.O; f.n_saves = d->n_saves;
        f.gid = g.renumbered && !part ? h->d_own_gid.as<int32_t>() : nullptr;     // (a partition's mse_time rows stay in its order: gathered below)
        f.save_div = part ? 1.0 : 0.0;                                            // (a partition's per-save SUMS: divided after the fold)
        f.sel = sel.empty() ? nullptr : (const int64_t*)(base + o_esel);
        f.n_val = n_val;
        f.mse_time = e->mse_time ? (float*)(base + o_emt) : nullptr;
        f.mse_save = e->mse_save ? (double*)(base + o_ems) : nullptr;
        f.vpart = (double*)(base + o_evp);
        HIPCHK(h, launch_eval_finish(f, h->stream));
        vpart.resize((size_t)save_error_blocks(n_val));
        HIPCHK(h, hipMemcpyAsync(vpart.data(), f.vpart, vpart.size() * 8, hipMemcpyDeviceToHost, h->stream));
        if (part) {
            // this rank's sums -- [n_saves][O] per-save sums (zeros when not wanted), then the val_loss numerator, the blocks' sums in
            // block order -- folded over the ranks in ascending order by one kernel on the gathered doubles (rank_fold_f64; not
            // allreduce_f64: only the host and local transports add in rank order there)
            const size_t ns = (size_t)d->n_saves * c.O;
            std::vector<double> head(ns + 1, 0.0);
            if (e->mse_save) HIPCHK(h, hipMemcpyAsync(head.data(), f.mse_save, ns * 8, hipMemcpyDeviceToHost, h->stream));
            HIPCHK(h, hipStreamSynchronize(h->stream));
            for (double v : vpart) head[ns] += v;
            if (int rc = rank_fold_f64(h, head.data(), (int64_t)head.size(), nullptr, 0, nullptr)) return rc;
            for (size_t i = 0; e->mse_save && i < ns; ++i) e->mse_save[i] = head[i] / (double)g.N;
            if (e->mse_time) if (int rc = gather_rows_global(h, f.mse_time, c.O, e->mse_time)) return rc;
            d->n_rhs = R.n_rhs;
            e->val_loss = head[ns] / (double)n_val_all;
            return MGN_OK;
        }
        if (e->mse_save) HIPCHK(h, hipMemcpyAsync(e->mse_save, f.mse_save, (size_t)d->n_saves * c.O * 8, hipMemcpyDeviceToHost, h->stream));
        if (e->mse_time) HIPCHK(h, hipMemcpyAsync(e->mse_time, f.mse_time, nb, hipMemcpyDefault, h->stream));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    d->n_rhs = R.n_rhs;
    if (e) {      // the blocks' sums in block order
        double s = 0.0;
        for (double v : vpart) s += v;
        e->val_loss = s / (double)n_val;
    }
    return MGN_OK;
}

}  // namespace

extern "C" int mgn_rollout(mgn_handle* h, mgn_rollout_desc* d) try {
    return rollout_solve(h, d, nullptr, "mgn_rollout");
} MGN_CATCH(h)

// the tableau of an *_erk entry point, before anything else
static int erk_checked(mgn_handle* h, const double* tab, const char* who) {
    if (mgn_erk_check(tab) != MGN_OK) return fail(h, MGN_E_ARG, "%s: the tableau does not pass mgn_erk_check", who);
    return MGN_OK;
}

extern "C" int mgn_rollout_erk(mgn_handle* h, mgn_rollout_desc* d, const double* tab, int32_t adaptive) try {
    if (!h) return MGN_E_ARG;
    if (int rc = erk_checked(h, tab, "mgn_rollout_erk")) return rc;
    return rollout_solve(h, d, nullptr, "mgn_rollout_erk", tab, adaptive);
} MGN_CATCH(h)

int mgn::rollout_eval_run(mgn_handle* h, mgn_rollout_desc* d, mgn_rollout_eval_desc* e, bool partitions, const double* tab, int32_t adaptive) {
    const char* who = tab ? "mgn_rollout_eval_erk" : "mgn_rollout_eval";
    if (tab)
        if (int rc = erk_checked(h, tab, who)) return rc;
    // the descriptor first (a host-only handle answers it too)
    if (!d || !e || !e->gt) return fail(h, MGN_E_ARG, "%s: null argument", who);
    if (e->n_gt < d->n_saves) return fail(h, MGN_E_ARG, "%s: n_gt = %d ground-truth frames for n_saves = %d saves", who, e->n_gt, d->n_saves);
    if (e->n_sel < 0 || (e->n_sel > 0 && !e->sel)) return fail(h, MGN_E_ARG, "%s: n_sel must be >= 0, and sel given when it is > 0", who);
    if (e->sel_index_base != 0 && e->sel_index_base != 1) return fail(h, MGN_E_ARG, "%s: sel_index_base must be 0 or 1", who);
    if (h->cfg.nranks != 1 && !partitions)
        return fail(h, MGN_E_UNSUPPORTED, "%s drives one partition: on a partitioned handle call mgn_rollout and reduce the solution on the host", who);
    if (h->have_graph) {
        const int64_t n = (int64_t)h->g.N * h->cfg.O;
        for (int64_t i = 0; i < e->n_sel; ++i) {
            const int64_t li = (int64_t)e->sel[i] - e->sel_index_base;
            if (li < 0 || li >= n)
                return fail(h, MGN_E_ARG, "%s: sel[%lld] = %d is outside the %lld elements of the [N][O] error array (index base %d)", who,
                            (long long)i, e->sel[i], (long long)n, e->sel_index_base);
        }
    }
    e->val_loss = 0.0;
    return rollout_solve(h, d, e, who, tab, adaptive);      // (without a graph it refuses before sel is read)
}

extern "C" int mgn_rollout_eval_erk(mgn_handle* h, mgn_rollout_desc* d, mgn_rollout_eval_desc* e, const double* tab, int32_t adaptive) try {
    if (!h || !tab) return MGN_E_ARG;
    return rollout_eval_run(h, d, e, false, tab, adaptive);
} MGN_CATCH(h)

extern "C" int mgn_rollout_eval(mgn_handle* h, mgn_rollout_desc* d, mgn_rollout_eval_desc* e) try {
    if (!h) return MGN_E_ARG;
    return rollout_eval_run(h, d, e, false);
} MGN_CATCH(h)

// ---- solver-based training (SolverTraining / MultipleShooting): loss and gradient of one solved window ------------------------------
// Forward: mgn_rollout's time loop on the resident right-hand side (the same launches, the same hipGraph replay), in the training form of
// the inflow overwrite (ode_func_train writes the inflow rows into a copy, reference src/solve.jl:101-117), storing the arrays the RHS saw.
// Backward: erk_sweep (mgn_train.cpp).  One edge set, fp32; the state in the engine's order throughout.  One partition
// on a rank handle; through the group (partitions = true) the state is the rows a rank owns, every VJP of the sweep runs the partitioned
// TrainPass, and the sweep's finish folds the ranks' loss sums and double gradient accumulators once (Sweep::finish, rank_fold_f64).
namespace {

// the inflow and the continuity weight
int solver_inflow_checks(mgn_handle* h, const mgn_rollout_desc* d, const char* who, float cont_weight) {
    if (int rc = inflow_checks(h, d, who)) return rc;
    if (d->inflow_data && d->n_frames < 1) return fail(h, MGN_E_ARG, "%s: inflow_data needs n_frames >= 1", who);
    if (!std::isfinite(cont_weight)) return fail(h, MGN_E_ARG, "%s: cont_weight must be finite", who);
    return MGN_OK;
}

// the fixed-step grid (TimeGrid::next) walked once on the host: K = round((t1 - t0) / dt) steps, and the step whose state each of the
// n_saves saves is (every one must be reached)
int fixed_grid(mgn_handle* h, const char* who, const TimeGrid& T, int n_saves, int64_t* K, std::vector<int64_t>& save_step) {
    const double steps = (T.t1 - T.t0) / T.dt;
    if (!(steps < 1e9)) return fail(h, MGN_E_ARG, "%s: %.3g steps", who, steps);
    *K = (int64_t)std::llround(steps);
    save_step.assign(1, 0);
    double t = T.t0;
    for (int64_t i = 0; i < *K && (int)save_step.size() < n_saves; ++i) {
        t = T.next(i, *K, t);
        while ((int)save_step.size() < n_saves && T.stop_time((int)save_step.size()) <= t + 0.25 * T.dt) save_step.push_back(i + 1);
    }
    if ((int)save_step.size() < n_saves)
        return fail(h, MGN_E_ARG, "%s: save point %d (t = %.9g) lies beyond the end of the solve (t1 = %.9g): every save must be reached", who,
                    (int)save_step.size(), T.stop_time((int)save_step.size()), T.t1);
    return MGN_OK;
}

// gt and cont_target (host or device, the caller's order) into the engine's order (gtl, ctl); loss_scale as given (lsd); tmp: [N][O] scratch
int solver_targets(mgn_handle* h, mgn_rollout_desc* d, const float* gt, const float* cont_target, const float* loss_scale, float* gtl, float* ctl,
                   float* lsd, float* tmp) {
    if (int rc = to_engine_order(h, gt, d->n_saves, gtl, tmp)) return rc;
    if (ctl)
        if (int rc = to_engine_order(h, cont_target, 1, ctl, tmp)) return rc;
    if (lsd) HIPCHK(h, hipMemcpyAsync(lsd, loss_scale, (size_t)h->cfg.O * 4, hipMemcpyDefault, h->stream));
    return MGN_OK;
}

// the reverse sweep of solve R: its accepted steps over their stored stage inputs (steps[n]: step n's s' arrays), its tableau and its saves.
// R.save_step is the plan the solve was given once all its saves are taken (saves_after pushes the plan's own entries; the shooting pass
// checks R.saved).  ybar: scratch [s' - 1][n]
SolverSweep sweep_setup(const Rollout& R, const std::vector<float*>& steps, float* ybar, const float* gt, const float* loss_scale,
                        const uint8_t* inflow, const float* cont_target, float* a, double* gacc) {
    SolverSweep S{};
    S.K = (int64_t)R.step_h.size(); S.steps = steps.data(); S.h = R.step_h.data(); S.xend = R.u; S.ybar = ybar;
    S.stages = R.tb->active(); S.b = R.tb->b; S.A = R.tb->A;
    S.saves = R.saves; S.save_step = R.save_step.data(); S.n_saves = R.d->n_saves;
    S.gt = gt; S.loss_scale = loss_scale; S.inflow = inflow; S.cont_target = cont_target;
    S.a = a; S.gacc = gacc;
    return S;
}

// mgn_solver_grad (o null: it has no options of its caller's), mgn_solver_grad_tsit5 and mgn_solver_grad_erk after their own checks, for
// tableau tb in the step mode o->adaptive names: the time grid, the forward loop keeping every accepted step's s' = s - fsal stage inputs
// in chunks on the handle, the targets, erk_sweep, the predicted saves
int solver_grad(mgn_handle* h, mgn_rollout_desc* d, mgn_solver_grad_opts* o, const Erk& tb, const char* who, const float* gt, const float* loss_scale,
                const float* cont_target, float cont_weight, float* grads, size_t n_grads, float* loss, bool partitions) {
    mgn_solver_grad_opts own{};
    const bool bounded = o != nullptr;      // the ceiling of 100000 accepted steps (maxiters) is the entry points' that take options
    if (!o) o = &own;
    const bool adaptive = o->adaptive & MGN_TSIT5_ADAPTIVE, dense = o->adaptive & MGN_TSIT5_DENSE_SAVES;
    const TimeGrid T(d);
    if (d->n_saves < 1 || !(T.sdt > 0.0) || !(T.t1 >= T.t0)) return fail(h, MGN_E_ARG, "%s: bad time grid", who);
    if (!adaptive && !(T.dt > 0.0)) return fail(h, MGN_E_ARG, bounded ? "%s: fixed steps need dt > 0" : "%s: Euler needs dt > 0", who);
    if (adaptive && !(T.dt >= 0.0)) return fail(h, MGN_E_ARG, "%s: dt must be >= 0 (0: the Hairer-Wanner start)", who);
    if (adaptive && !(d->abstol > 0.f && d->reltol > 0.f)) return fail(h, MGN_E_ARG, "%s: tolerances must be > 0", who);
    if (int rc = solver_inflow_checks(h, d, who, cont_weight)) return rc;
    o->n_steps = 0;
    o->stored_bytes = 0;
    int64_t K = 0;                       // fixed steps: the step count; adaptive: the accepted steps, after the solve
    std::vector<int64_t> plan;
    if (!adaptive && !dense) {
        if (int rc = fixed_grid(h, who, T, d->n_saves, &K, plan)) return rc;
    } else if (T.stop_time(d->n_saves - 1) > T.t1 + 1e-5 * T.sdt) {
        return fail(h, MGN_E_ARG, "%s: save point %d (t = %.9g) lies beyond the end of the solve (t1 = %.9g): every save must be reached", who,
                    d->n_saves - 1, T.stop_time(d->n_saves - 1), T.t1);
    }
    // fp32, one partition (partitions: or a partitioned mesh with one edge set and a communicator), parameter count; the training arena.
    // These were the last checks: on a partitioned mesh no rank refuses after its peers have entered a collective
    if (int rc = partitions ? solver_prepare_partitions(h, who, n_grads) : solver_prepare(h, n_grads)) return rc;
    const mgn_config& c = h->cfg;
    const bool part = c.nranks != 1;       // every rank integrates and sweeps the rows it owns (rollout_solve's state)
    const int32_t N = part ? h->g.n_own : h->g.N;
    const int O = c.O;
    invalidate_static(h);
    Rollout R(h, d, T, true, N, h->g.N);
    R.tb = &tb;
    const size_t nb = (size_t)R.n * 4;
    const size_t P = h->params.size();
    const int ablk = solver_adjoint_blocks(N, O);
    const size_t fb = d->inflow_data ? (size_t)d->n_frames * nb : 0, sb = (size_t)d->n_saves * nb;
    const size_t eb = tile_floats(h->es[0].ntiles_e, c.L) * 4;
    Arena a;
    const SolveWs ws = carve_solve(a, nb, tb.s, tb.fsal, !adaptive && !dense, d->inflow_mask != nullptr);
    const size_t o_fr = a.take(fb), o_sv = a.take(sb), o_mask = a.take((size_t)N), o_pe = a.take(adaptive ? errnorm_partials() * sizeof(double) : 0);
    R.elat0_off = a.take(eb);
    const size_t o_gt = a.take(sb), o_ct = a.take(cont_target ? nb : 0), o_ls = a.take((size_t)O * 4), o_a = a.take(nb),
                 o_tmp = a.take(part ? (size_t)h->g.N * O * 4 : nb), o_yb = a.take((size_t)(tb.active() - 1) * nb), o_gacc = a.take(P * sizeof(double)),
                 o_part = a.take((size_t)(d->n_saves + 1) * 2 * ablk * sizeof(double));
    const size_t o_dn = a.take(dense ? 7 * nb : 0);      // dense saves: the sweep's sums of a step's interpolated saves (SolverSweep::dense)
    if (int rc = dense ? ensure_or_fail(h, h->ode, a.off, "%s: %.3f GB for the call's buffers (%.3f GB of them the sums of the interpolated saves)", who,
                                        (double)a.off * 1e-9, (double)(7 * nb) * 1e-9)
                       : ensure_or_fail(h, h->ode, a.off, "%s: %.3f GB for the call's buffers", who, (double)a.off * 1e-9))
        return rc;
    char* base = h->ode.as<char>();
    R.bind(base, ws);
    R.frames = d->inflow_data ? (float*)(base + o_fr) : nullptr;
    R.saves = (float*)(base + o_sv);
    R.mask = d->inflow_mask ? (uint8_t*)(base + o_mask) : nullptr;
    R.partial = adaptive ? (double*)(base + o_pe) : nullptr;
    if (int rc = upload_engine_order(h, d, R.u, R.frames, R.mask)) return rc;
    if (int rc = upload_statics(h, d, d->x0, base + R.elat0_off, eb)) return rc;

    // the stored stage inputs, step n's s' [N][O] arrays (Euler: one, Tsit5: six) at steps[n], carved out of chunks kept on the handle and
    // grown geometrically (never reallocated: a stored step does not move)
    const size_t stepb = (size_t)tb.active() * nb;
    const size_t denseb = dense ? 7 * nb : 0;      // counted with the stored stage inputs (max_store_bytes, stored_bytes)
    const int64_t max_steps = 100000;
    std::vector<float*> steps;
    size_t chunk = 0, used_in_chunk = 0;
    const Rollout::Slot slot = [&](int64_t n, float** out) -> int {
        while ((int64_t)steps.size() <= n) {
            if (bounded && (int64_t)steps.size() >= max_steps)
                return fail(h, MGN_E_STATE, "%s: more than %lld accepted steps (maxiters)", who, (long long)max_steps);
            if (o->max_store_bytes && (size_t)(steps.size() + 1) * stepb + denseb > o->max_store_bytes)
                return fail(h, MGN_E_OOM, "%s: step %lld needs %zu bytes of stored stage inputs%s, beyond max_store_bytes = %zu", who,
                            (long long)steps.size(), (size_t)(steps.size() + 1) * stepb + denseb, dense ? " and sums of the interpolated saves" : "",
                            o->max_store_bytes);
            DevBuf* cb = chunk < h->stage_store.size() ? h->stage_store[chunk].get() : nullptr;
            if (cb && used_in_chunk + stepb <= cb->bytes) {
                steps.push_back(reinterpret_cast<float*>(cb->as<char>() + used_in_chunk));
                used_in_chunk += stepb;
                continue;
            }
            if (cb && used_in_chunk > 0) { ++chunk; used_in_chunk = 0; continue; }
            // a new chunk (or an earlier call's that holds no step of this size, regrown in place): as many steps as are stored so far (at
            // least 8; a fixed-step solve: all it has left), within max_store_bytes
            size_t want = (size_t)std::max<int64_t>((adaptive || dense) ? std::max<int64_t>((int64_t)steps.size(), 8) : K - (int64_t)steps.size(), 1);
            if (o->max_store_bytes) want = std::min(want, (o->max_store_bytes - denseb) / stepb - steps.size());
            if (want > (SIZE_MAX / 2) / stepb) return fail(h, MGN_E_OOM, "%s: %zu stored steps overflow the address space", who, want);
            if (!cb) {
                h->stage_store.push_back(std::make_unique<DevBuf>());
                cb = h->stage_store.back().get();
            }
            if (int rc = ensure_or_fail(h, *cb, want * stepb, "%s: step %lld: %.3f GB more for the stored stage inputs (%.3f GB stored)", who,
                                        (long long)steps.size(), (double)(want * stepb) * 1e-9, (double)(steps.size() * stepb) * 1e-9))
                return rc;
            used_in_chunk = 0;
        }
        *out = steps[n];
        return MGN_OK;
    };

    d->n_accept = d->n_reject = 0;
    R.dense = dense;
    if (int rc = adaptive ? R.erk_adaptive(who, &slot) : dense ? R.tsit5_fixed_dense(&slot) : R.erk_fixed(K, plan, &slot)) return rc;
    d->n_rhs = R.n_rhs;
    K = (int64_t)R.step_h.size();
    o->n_steps = (int32_t)K;
    o->stored_bytes = (size_t)K * stepb + denseb;
    for (int64_t i = 0; i < K && i < o->step_cap; ++i) {
        if (o->step_t) o->step_t[i] = R.step_t[i];
        if (o->step_h) o->step_h[i] = R.step_h[i];
    }

    float* gtl = (float*)(base + o_gt);
    float* ctl = cont_target ? (float*)(base + o_ct) : nullptr;
    float* lsd = loss_scale ? (float*)(base + o_ls) : nullptr;
    if (int rc = solver_targets(h, d, gt, cont_target, loss_scale, gtl, ctl, lsd, (float*)(base + o_tmp))) return rc;

    SolverSweep S = sweep_setup(R, steps, (float*)(base + o_yb), gtl, lsd, R.mask, ctl, (float*)(base + o_a), (double*)(base + o_gacc));
    S.cont_weight = ctl ? cont_weight : 0.f;
    S.onehot = d->node_type_onehot; S.ef_raw = d->ef_raw; S.val_mask = d->val_mask;
    S.part = (double*)(base + o_part); S.grads = grads; S.loss = loss;
    if (dense) {      // the plan of the interpolated saves is R.save_step / R.save_theta
        S.theta = R.save_theta.data();
        S.zend = R.rhs_input(R.u, R.za);      // z_{K,1}: what stage 7 of the last accepted trial was evaluated on
        S.dense = (float*)(base + o_dn);
    }
    if (int rc = erk_sweep(h, S)) return rc;
    if (d->out && part) {      // the predicted saves, complete on every rank (every rank was given d->out, or none)
        for (int i = 0; i < d->n_saves; ++i)
            if (int rc = gather_rows_global(h, R.saves + (size_t)i * R.n, O, d->out + (size_t)i * h->g.N * O)) return rc;
    } else if (d->out) {       // the predicted saves in the caller's order
        if (int rc = saves_to_caller(h, R.saves, d->n_saves, d->out)) return rc;
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return MGN_OK;
}

// the checks mgn_solver_grad and mgn_solver_grad_tsit5 share before their solver's
int solver_checks(mgn_handle* h, mgn_rollout_desc* d, const char* who, const float* gt, float* grads, float* loss, bool partitions) {
    if (int rc = solver_state_checks(h, who, partitions)) return rc;
    if (!d || !gt || !grads || !loss || !d->x0) return fail(h, MGN_E_ARG, "%s: null argument", who);
    return solver_static_checks(h, d, who);
}

}  // namespace

// mgn_solver_grad (solver MGN_SOLVER_EULER; o unused) and mgn_solver_grad_tsit5 (MGN_SOLVER_TSIT5) behind their symbols, and behind
// mgn_group_solver_grad* (partitions)
int mgn::solver_grad_run(mgn_handle* h, mgn_rollout_desc* d, mgn_solver_grad_opts* o, int32_t solver, const float* gt, const float* loss_scale,
                         const float* cont_target, float cont_weight, float* grads, size_t n_grads, float* loss, bool partitions) {
    const bool tsit5 = solver == MGN_SOLVER_TSIT5;
    const char* who = tsit5 ? "mgn_solver_grad_tsit5" : "mgn_solver_grad";
    // the step mode first: a host-only handle answers it too
    if (tsit5 && o && (o->adaptive & ~(MGN_TSIT5_ADAPTIVE | MGN_TSIT5_DENSE_SAVES)))
        return fail(h, MGN_E_ARG, "%s: adaptive = %d: the step mode is MGN_TSIT5_ADAPTIVE | MGN_TSIT5_DENSE_SAVES, nothing else", who, o->adaptive);
    if (int rc = solver_checks(h, d, who, gt, grads, loss, partitions)) return rc;
    if (!tsit5) {
        if (d->solver == 1) return fail(h, MGN_E_UNSUPPORTED, "mgn_solver_grad: the discrete adjoint is built for fixed-step Euler (solver 0); Tsit5 is mgn_solver_grad_tsit5");
        if (d->solver != 0) return fail(h, MGN_E_ARG, "mgn_solver_grad: solver must be 0 (Euler)");
        return solver_grad(h, d, nullptr, erk_euler(), who, gt, loss_scale, cont_target, cont_weight, grads, n_grads, loss, partitions);
    }
    if (!o) return fail(h, MGN_E_ARG, "%s: null argument", who);
    if (d->solver != 1) return fail(h, MGN_E_ARG, "%s: solver must be 1 (Tsit5)", who);
    if (o->step_cap < 0 || (o->step_cap > 0 && !o->step_t && !o->step_h)) return fail(h, MGN_E_ARG, "%s: step_cap needs step_t or step_h", who);
    return solver_grad(h, d, o, erk_tsit5(), who, gt, loss_scale, cont_target, cont_weight, grads, n_grads, loss, partitions);
}

extern "C" int mgn_solver_grad(mgn_handle* h, mgn_rollout_desc* d, const float* gt, const float* loss_scale, const float* cont_target, float cont_weight,
                    float* grads, size_t n_grads, float* loss) try {
    if (!h) return MGN_E_ARG;
    return solver_grad_run(h, d, nullptr, MGN_SOLVER_EULER, gt, loss_scale, cont_target, cont_weight, grads, n_grads, loss, false);
} MGN_CATCH(h)

// mgn_solver_grad_tsit5's loss and gradient for any explicit Runge-Kutta tableau with at most six active stages, fixed steps only: the
// grid and saves of mgn_rollout_erk(adaptive = 0) in the training form, the s' stage inputs of every step kept in h->stage_store, then
// the same table-driven sweep.  d->solver is not read.
extern "C" int mgn_solver_grad_erk(mgn_handle* h, mgn_rollout_desc* d, const double* tab, mgn_solver_grad_opts* o, const float* gt,
                                   const float* loss_scale, const float* cont_target, float cont_weight, float* grads, size_t n_grads,
                                   float* loss) try {
    static const char* who = "mgn_solver_grad_erk";
    if (!h) return MGN_E_ARG;
    if (int rc = erk_checked(h, tab, who)) return rc;
    // the step mode and the stage count next: a host-only handle answers them too
    if (!o) return fail(h, MGN_E_ARG, "%s: null argument", who);
    if (o->adaptive != 0)
        return fail(h, MGN_E_UNSUPPORTED, "%s: adaptive = %d: fixed steps only (adaptive training is mgn_solver_grad_tsit5's, with Tsit5)", who, o->adaptive);
    const Erk erk = erk_unpack(tab);
    if (erk.active() > 6) return fail(h, MGN_E_UNSUPPORTED, "%s: %d active stages; the sweep holds six", who, erk.active());
    if (int rc = solver_checks(h, d, who, gt, grads, loss, false)) return rc;
    if (o->step_cap < 0 || (o->step_cap > 0 && !o->step_t && !o->step_h)) return fail(h, MGN_E_ARG, "%s: step_cap needs step_t or step_h", who);
    const TimeGrid T(d);
    if (T.dt > 0.0 && T.sdt > 0.0) {      // (solver_grad refuses the rest of a bad grid)
        const double per = T.sdt / T.dt, m = std::round(per);
        if (!(m >= 1.0) || std::fabs(per - m) > 1e-6 * m)
            return fail(h, MGN_E_ARG, "%s: saves_dt / dt = %.9g is not an integer >= 1: a general tableau has no dense output", who, per);
    }
    return solver_grad(h, d, o, erk, who, gt, loss_scale, cont_target, cont_weight, grads, n_grads, loss, false);
} MGN_CATCH(h)

// Tsit5: mgn_rollout's adaptive loop (Rollout::erk_adaptive, StepControl) or fixed steps on the fixed grid (Rollout::erk_fixed), in
// the training form (za / zs / z7), keeping the six stage inputs of every accepted step in h->stage_store; then erk_sweep.
extern "C" int mgn_solver_grad_tsit5(mgn_handle* h, mgn_rollout_desc* d, mgn_solver_grad_opts* o, const float* gt, const float* loss_scale,
                          const float* cont_target, float cont_weight, float* grads, size_t n_grads, float* loss) try {
    if (!h) return MGN_E_ARG;
    return solver_grad_run(h, d, o, MGN_SOLVER_TSIT5, gt, loss_scale, cont_target, cont_weight, grads, n_grads, loss, false);
} MGN_CATCH(h)

// ---- MultipleShooting as one batch (mgn_shooting_grad) ----------------------------------------------------------------------------------
// The windows of one MultipleShooting loss are independent (each starts from gt; the continuity term couples a window to gt only), so
// windows with the same step plan are solved together on a companion engine holding B copies of the graph: one solve of a block-diagonal
// graph per pass instead of B launch-bound solves.  Per window the arithmetic is that of mgn_solver_grad / mgn_solver_grad_tsit5 (fixed
// steps); the loss partials and the gradient accumulate over all passes and are finalised once.
void mgn::shoot_release(mgn_engine* h) {
    if (!h) return;
    for (auto& k : h->shoot_kids) mgn_destroy(k.e);
    h->shoot_kids.clear();
    h->shoot.release();
}

namespace {

const char* const shoot_who = "mgn_shooting_grad";

struct ShootGroup {
    int64_t K = 0;
    std::vector<int64_t> save_step;          // n_saves entries, the same for every window of the group
    std::vector<int32_t> win;                // its windows, ascending
    std::vector<std::vector<int32_t>> fr;    // per window: the inflow frame of every right-hand side evaluation (no inflow mask: empty)
    size_t ftab_off = 0;                     // [n_evals][win.size()] in the int table
    TimeGrid tg;                             // its first window's
};

}  // namespace

// The companion of B copies of h's graph in h's engine order (row w N + i = copy w's engine row i), not renumbered, on h's stream and with
// h's parameters (packed again only when they changed).  inference: what a solve on it needs as well -- the inference latents, h's
// normalisers (a blocking copy where the device rewrote them) and the inference weight layouts.  The batched training step
// (mgn_step_datapoints) takes normalised inputs and trains: it asks for none of the three.
int mgn::companion_engine(mgn_handle* h, int32_t B, const char* who, bool inference, mgn_engine** out) {
    mgn_engine::ShootKid* kid = nullptr;
    for (auto& k : h->shoot_kids)
        if (k.b == B) kid = &k;
    if (!kid) {
        if (h->shoot_kids.size() >= 2) {     // the oldest size goes
            mgn_destroy(h->shoot_kids.front().e);
            h->shoot_kids.erase(h->shoot_kids.begin());
        }
        const LocalGraph& g = h->g;
        const int32_t N = g.N;
        const EdgeTopo& t = g.set[0];
        const int64_t E = t.e_local;
        if ((int64_t)B * N > INT32_MAX || (int64_t)B * E > INT32_MAX) return fail(h, MGN_E_ARG, "%s: %d windows of %d nodes overflow int32 node ids", who, B, N);
        mgn_engine* c = nullptr;
        mgn_config cfg = h->cfg;
        if (mgn_create(&cfg, &c) != MGN_OK) return fail(h, MGN_E_HIP, "%s: companion engine: %s", who, mgn_last_error(nullptr));
        c->companion = true;
        std::vector<int32_t> snd((size_t)B * E), rcv((size_t)B * E);
        for (int32_t w = 0; w < B; ++w)
            for (int64_t j = 0; j < E; ++j) {
                snd[(size_t)w * E + j] = w * N + t.snd[j];
                rcv[(size_t)w * E + j] = w * N + t.rcv[j];
            }
        EdgeList sets[MAX_EDGE_SETS];
        sets[0] = {(int64_t)B * E, snd.data(), rcv.data(), 0};
        int rc = rebuild_graph(c, B * N, sets, nullptr, 0, false, who, nullptr, 0);
        if (rc) {
            rc = fail(h, rc, "%s: companion graph: %s", who, c->err.c_str());
            mgn_destroy(c);
            return rc;
        }
        c->have_graph = true;
        h->shoot_kids.push_back({B, c, 0, false, false});
        kid = &h->shoot_kids.back();
        // the copies keep h's engine order: no renumbering, edges in the replicated (receiver-sorted, stable) order
        const LocalGraph& cg = c->g;
        bool same = !cg.renumbered && cg.n_own == B * N && cg.set[0].e_local == (int64_t)B * E;
        for (int32_t i = 0; same && i < cg.n_own; ++i) same = cg.own_gid[i] == i;
        for (int64_t j = 0; same && j < cg.set[0].e_local; ++j) same = cg.set[0].edge_gid[j] == j;
        if (!same) return fail(h, MGN_E_STATE, "%s: the companion graph does not keep the replicated order", who);
    }
    mgn_engine* c = kid->e;
    if (c->stream != h->stream)
        if (mgn_set_stream(c, (void*)h->stream) != MGN_OK) return fail(h, MGN_E_HIP, "%s: companion stream: %s", who, c->err.c_str());
    if (!kid->params_set || kid->params_gen != h->params_gen) {      // parameters only when they changed
        // device to device, on the stream both share: whichever door h's parameters came through, its resident copy is the source
        const float* dp = nullptr;
        if (int rc = dev_params(h, &dp)) return rc;
        if (set_params_resident(c, dp, h->params.size(), who) != MGN_OK) return fail(h, MGN_E_STATE, "%s: companion parameters: %s", who, c->err.c_str());
        kid->params_set = true;
        kid->params_gen = h->params_gen;
    }
    *out = c;
    if (!inference) return MGN_OK;
    if (!kid->latents) {
        if (int rc = alloc_latents(c)) return fail(h, rc, "%s: companion graph: %s", who, c->err.c_str());
        kid->latents = true;
    }
    if (int rc = sync_norms_host(h)) return rc;
    if (c->norms_host != h->norms_host || c->have_nnorm != h->have_nnorm || c->have_enorm != h->have_enorm || c->have_onorm != h->have_onorm) {
        const mgn_config& k = h->cfg;
        const float* v = h->norms_host.data();
        const float* ne = v + 2 * k.Fn;
        const float* no = ne + 2 * k.Fe;
        if (mgn_set_norms(c, h->have_nnorm ? v : nullptr, h->have_nnorm ? v + k.Fn : nullptr, h->have_enorm ? ne : nullptr,
                          h->have_enorm ? ne + k.Fe : nullptr, h->have_onorm ? no : nullptr, h->have_onorm ? no + k.O : nullptr) != MGN_OK)
            return fail(h, MGN_E_STATE, "%s: companion normalisers: %s", who, c->err.c_str());
        c->norms_host = h->norms_host;
    }
    if (int rc = need(c, true, true, true, true)) return fail(h, rc, "%s: companion: %s", who, c->err.c_str());
    return MGN_OK;
}

namespace {

// the companion for passes of B windows: parameters and normalisers brought up to date
int shoot_companion(mgn_handle* h, int32_t B, mgn_engine** out) { return companion_engine(h, B, shoot_who, true, out); }

// the static inputs of a companion pass: h's engine-order arrays replicated B times on the device, the edges encoded once into elat0
int shoot_statics(mgn_engine* c, int32_t B, int32_t N, const float* oh, const float* vm, const float* ef, char* elat0, size_t eb) {
    const mgn_config& k = c->cfg;
    const int W1 = k.Fn - k.O, Fe = k.Fe;
    const int64_t E = c->g.set[0].e_local / B, rows = (int64_t)B * N;
    c->in_wa = k.O;
    c->in_wb = W1;
    c->in_local = true;                      // (the state slot d_nfA is never read: every right-hand side reads srcA_override)
    HIPCHK(c, c->d_nfA.ensure(16));
    HIPCHK(c, c->d_nfB.ensure((size_t)rows * (W1 > 0 ? W1 : 1) * 4));
    if (W1 > 0) HIPCHK(c, launch_shoot_gather(c->d_nfB.as<float>(), oh, rows * W1, (int64_t)N * W1, 1, nullptr, nullptr, 0, c->stream));
    c->have_mask = vm != nullptr;
    if (vm) {
        HIPCHK(c, c->d_mask.ensure((size_t)rows * 4));
        HIPCHK(c, launch_shoot_gather(c->d_mask.as<float>(), vm, rows, N, 1, nullptr, nullptr, 0, c->stream));
    }
    HIPCHK(c, c->es[0].d_ef.ensure((size_t)B * E * Fe * 4 + 16));
    if (E > 0) HIPCHK(c, launch_shoot_gather(c->es[0].d_ef.as<float>(), ef, (int64_t)B * E * Fe, E * Fe, 1, nullptr, nullptr, 0, c->stream));
    if (int rc = encode_impl(c, true, false, true)) return rc;
    HIPCHK(c, hipMemcpyAsync(elat0, c->es[0].Elat.p, eb, hipMemcpyDeviceToDevice, c->stream));
    return MGN_OK;
}

struct ShootPass { int32_t grp, j0, B; size_t idx_off, cw_off; };

// what the steps of one mgn_shooting_grad call hand on: the checked call, the host plan (shoot_plans), the staging on h->shoot (shoot_stage)
struct ShootCtx {
    mgn_handle* h; mgn_rollout_desc* d; mgn_shooting_desc* s;
    float cont_weight; size_t n_grads;
    TimeGrid DG;                             // (its time type, dt and saves_dt; every window has its own t0 and t1)
    const Erk& tb;                           // d->solver's tableau (the windows take fixed steps)
    bool inflow;
    int32_t N; int O, W1, Fe; int64_t E, nN;
    mgn_rollout_desc dw;                     // a pass's descriptor: d with its group's n_saves
    std::vector<ShootGroup> groups;
    std::vector<ShootPass> passes;
    std::vector<int32_t> itab;               // int32 tables: per group the frame table, per pass x0 [B] | save targets [n_saves][B] | continuity [B]
    std::vector<float> cwtab;
    std::vector<int64_t> out_row;            // the first output save of every window
    int32_t Bmax = 1;
    int ld = 0;
    char* sbase = nullptr;
    size_t o_oh = 0, o_vm = 0, o_ef = 0, o_out = 0, o_gf = 0;
    float *gtl = nullptr, *frl = nullptr, *lsd = nullptr; uint8_t* mkl = nullptr; double *gacc = nullptr, *lacc = nullptr;
    const int32_t* itd = nullptr; const float* cwd = nullptr;
    // host arrays that asynchronous copies read, and the captured right-hand sides: alive until the final synchronisation
    std::vector<float> hs, zero_x0;          // the statics of companion passes in the engine's order; the encoder's unused state slot of a one-window pass
    std::vector<std::unique_ptr<Rollout>> keep_alive;
    ShootCtx(mgn_handle* h_, mgn_rollout_desc* d_, mgn_shooting_desc* s_, float cw, size_t ng)
        : h(h_), d(d_), s(s_), cont_weight(cw), n_grads(ng), DG(d_), tb(d_->solver == MGN_SOLVER_EULER ? erk_euler() : erk_tsit5()), inflow(d_->inflow_mask != nullptr), N(h_->g.N), O(h_->cfg.O),
          W1(h_->cfg.Fn - O), Fe(h_->cfg.Fe), E(h_->g.set[0].e_local), nN((int64_t)N * O), dw(*d_) {}
};

// The times of the right-hand side evaluations of K fixed steps, in the order Rollout::erk_first / erk_trial make them.  FSAL: k1 once up
// front, and the last stage (z_{n+1,1}) sees t_{n+1}; otherwise stage 1 at t every step.  Stages 2 .. s at tt(t + tt(c_i dt))
template <typename F>
int erk_eval_times(const Erk& e, const TimeGrid& T, int64_t K, F&& push) {
    double t = T.t0;
    if (e.fsal)
        if (int rc = push(t)) return rc;
    for (int64_t i = 0; i < K; ++i) {
        const double tn = T.next(i, K, t);
        if (!e.fsal)
            if (int rc = push(t)) return rc;
        for (int sidx = 1; sidx < e.s; ++sidx)
            if (int rc = push(e.fsal && sidx == e.s - 1 ? tn : T.tt(t + T.tt(e.c[sidx] * T.dt)))) return rc;
        t = tn;
    }
    return MGN_OK;
}

// ---- plans on the host: every window walks the single-window grid; identical plans form a group; then the passes and their tables
int shoot_plans(ShootCtx& X) {
    mgn_handle* h = X.h; mgn_rollout_desc* d = X.d; mgn_shooting_desc* s = X.s;
    for (int32_t w = 0; w < s->n_windows; ++w) {
        TimeGrid T = X.DG;
        T.t0 = T.tt(s->t0[w]);
        T.t1 = T.tt(s->t1[w]);
        if (!(T.t1 >= T.t0)) return fail(h, MGN_E_ARG, "%s: window %d: t1 < t0", shoot_who, w);
        char ww[64];
        snprintf(ww, sizeof ww, "%s: window %d", shoot_who, w);
        int64_t K;
        std::vector<int64_t> ss;
        if (int rc = fixed_grid(h, ww, T, s->last[w] - s->first[w] + 1, &K, ss)) return rc;
        std::vector<int32_t> fr;
        if (X.inflow) {      // the frame of every right-hand side evaluation, in the order the solve makes them
            const Rollout P(h, d, T);        // (its frame rule only)
            auto push = [&](double t) -> int {
                int64_t f;
                if (int rc = P.frame_index(t, &f)) return rc;
                fr.push_back((int32_t)f);
                return MGN_OK;
            };
            if (int rc = erk_eval_times(X.tb, T, K, push)) return rc;
        }
        int32_t gi = -1;
        for (size_t q = 0; q < X.groups.size() && gi < 0; ++q)
            if (X.groups[q].K == K && X.groups[q].save_step == ss) gi = (int32_t)q;
        if (gi < 0) {
            gi = (int32_t)X.groups.size();
            X.groups.push_back({K, ss, {}, {}, 0, T});
        }
        X.groups[gi].win.push_back(w);
        X.groups[gi].fr.push_back(std::move(fr));
    }

    // passes: a group's windows in chunks of at most `cap` (sizes as even as the cap allows)
    int64_t cap = std::max<int64_t>(1, (s->max_batch_nodes > 0 ? s->max_batch_nodes : ((int64_t)1 << 20)) / std::max<int32_t>(X.N, 1));
    if (s->max_windows_per_pass > 0) cap = std::min<int64_t>(cap, s->max_windows_per_pass);
    if (h->cfg.ln_dims == MGN_LN_ALL) cap = 1;   // a whole-array LayerNorm would couple the copies
    X.out_row.assign(s->n_windows + 1, 0);
    for (int32_t w = 0; w < s->n_windows; ++w) X.out_row[w + 1] = X.out_row[w] + (s->last[w] - s->first[w] + 1);
    for (size_t q = 0; q < X.groups.size(); ++q) {
        ShootGroup& G = X.groups[q];
        const int32_t nw = (int32_t)G.win.size();
        if (X.inflow) {
            G.ftab_off = X.itab.size();
            const size_t ne = G.fr[0].size();
            for (size_t e = 0; e < ne; ++e)
                for (int32_t j = 0; j < nw; ++j) X.itab.push_back(G.fr[j][e]);
        }
        const int32_t np = (int32_t)((nw + cap - 1) / cap);
        for (int32_t p = 0, j0 = 0; p < np; ++p) {
            const int32_t B = nw / np + (p < nw % np ? 1 : 0);
            ShootPass ps{(int32_t)q, j0, B, X.itab.size(), X.cwtab.size()};
            const int ns = (int)G.save_step.size();
            for (int32_t j = 0; j < B; ++j) X.itab.push_back(s->first[G.win[j0 + j]]);
            for (int sv = 0; sv < ns; ++sv)
                for (int32_t j = 0; j < B; ++j) X.itab.push_back(s->first[G.win[j0 + j]] + sv);
            for (int32_t j = 0; j < B; ++j) {
                const int32_t w = G.win[j0 + j];
                X.itab.push_back(w + 1 < s->n_windows ? s->first[w + 1] : s->first[w]);
                X.cwtab.push_back(w + 1 < s->n_windows ? X.cont_weight : 0.f);
            }
            X.passes.push_back(ps);
            X.Bmax = std::max(X.Bmax, B);
            j0 += B;
        }
    }
    return MGN_OK;
}

// ---- the call's staging on the handle: gt (engine order), frames, masks, statics, tables, accumulators
int shoot_stage(ShootCtx& X, const float* gt, const float* loss_scale) {
    mgn_handle* h = X.h; mgn_rollout_desc* d = X.d; mgn_shooting_desc* s = X.s;
    const size_t P_ = h->params.size();
    X.ld = solver_adjoint_blocks((int64_t)X.Bmax * X.N, X.O);
    const bool any_batch = X.Bmax > 1;
    const size_t gtb = (size_t)s->n_gt * X.nN * 4;
    const size_t fb = X.inflow ? (size_t)d->n_frames * X.nN * 4 : 0;
    Arena a;
    const size_t o_gt = a.take(gtb), o_gtc = a.take(h->g.renumbered ? gtb : 0), o_fr = a.take(fb), o_mk = a.take(X.inflow ? (size_t)X.N : 0);
    X.o_oh = a.take(any_batch ? (size_t)X.N * X.W1 * 4 : 0); X.o_vm = a.take(any_batch && d->val_mask ? (size_t)X.N * 4 : 0);
    X.o_ef = a.take(any_batch ? (size_t)X.E * X.Fe * 4 : 0); X.o_out = a.take(d->out ? (size_t)X.out_row[s->n_windows] * X.nN * 4 : 0);
    const size_t o_gacc = a.take(P_ * 8), o_lacc = a.take((size_t)2 * X.ld * 8);
    X.o_gf = a.take(P_ * 4);
    const size_t o_ls = a.take((size_t)X.O * 4), o_it = a.take(X.itab.size() * 4), o_cw = a.take(X.cwtab.size() * 4);
    if (int rc = ensure_or_fail(h, h->shoot, a.off, "%s: %.3f GB for the call's staging", shoot_who, (double)a.off * 1e-9)) return rc;
    X.sbase = h->shoot.as<char>();
    X.gtl = (float*)(X.sbase + o_gt);
    X.frl = X.inflow ? (float*)(X.sbase + o_fr) : nullptr;
    X.mkl = X.inflow ? (uint8_t*)(X.sbase + o_mk) : nullptr;
    X.gacc = (double*)(X.sbase + o_gacc);
    X.lacc = (double*)(X.sbase + o_lacc);
    X.lsd = loss_scale ? (float*)(X.sbase + o_ls) : nullptr;
    X.itd = (const int32_t*)(X.sbase + o_it);
    X.cwd = (const float*)(X.sbase + o_cw);
    const int32_t* ngid = h->d_own_gid.as<int32_t>();
    if (!h->g.renumbered) {
        HIPCHK(h, hipMemcpyAsync(X.gtl, gt, gtb, hipMemcpyDefault, h->stream));
    } else {
        HIPCHK(h, hipMemcpyAsync(X.sbase + o_gtc, gt, gtb, hipMemcpyDefault, h->stream));
        HIPCHK(h, launch_shoot_gather(X.gtl, (const float*)(X.sbase + o_gtc), (int64_t)s->n_gt * X.nN, X.nN, s->n_gt, nullptr, ngid, X.O, h->stream));
    }
    // host arrays (as mgn_rollout takes them) into the engine's order: frames, inflow mask, and the statics of companion passes (the node
    // order of one partition: own_gid)
    if (int rc = upload_engine_order(h, d, nullptr, X.frl, X.mkl)) return rc;
    if (any_batch) {
        X.hs.resize((size_t)X.N * X.W1 + (d->val_mask ? (size_t)X.N : 0) + (size_t)X.E * X.Fe);
        float* ho = X.hs.data();
        float* hv = ho + (size_t)X.N * X.W1;
        float* he = hv + (d->val_mask ? (size_t)X.N : 0);
        for (int32_t i = 0; i < X.N; ++i) {
            const size_t gi = (size_t)h->g.own_gid[i];
            if (X.W1 > 0) memcpy(ho + (size_t)i * X.W1, d->node_type_onehot + gi * X.W1, (size_t)X.W1 * 4);
            if (d->val_mask) hv[i] = d->val_mask[gi];
        }
        for (int64_t j = 0; j < X.E; ++j) memcpy(he + (size_t)j * X.Fe, d->ef_raw + (size_t)h->g.set[0].edge_gid[j] * X.Fe, (size_t)X.Fe * 4);
        if (X.W1 > 0) HIPCHK(h, hipMemcpyAsync(X.sbase + X.o_oh, ho, (size_t)X.N * X.W1 * 4, hipMemcpyHostToDevice, h->stream));
        if (d->val_mask) HIPCHK(h, hipMemcpyAsync(X.sbase + X.o_vm, hv, (size_t)X.N * 4, hipMemcpyHostToDevice, h->stream));
        if (X.E > 0) HIPCHK(h, hipMemcpyAsync(X.sbase + X.o_ef, he, (size_t)X.E * X.Fe * 4, hipMemcpyHostToDevice, h->stream));
    }
    if (!X.itab.empty()) HIPCHK(h, hipMemcpyAsync(X.sbase + o_it, X.itab.data(), X.itab.size() * 4, hipMemcpyHostToDevice, h->stream));
    if (!X.cwtab.empty()) HIPCHK(h, hipMemcpyAsync(X.sbase + o_cw, X.cwtab.data(), X.cwtab.size() * 4, hipMemcpyHostToDevice, h->stream));
    if (X.lsd) HIPCHK(h, hipMemcpyAsync(X.lsd, loss_scale, (size_t)X.O * 4, hipMemcpyDefault, h->stream));
    HIPCHK(h, hipMemsetAsync(X.gacc, 0, P_ * 8, h->stream));
    HIPCHK(h, hipMemsetAsync(X.lacc, 0, (size_t)2 * X.ld * 8, h->stream));
    X.zero_x0.assign((size_t)X.nN, 0.f);
    return MGN_OK;
}

// ---- one pass: B windows of a group as one state on h itself (B = 1) or on the companion of B copies; solve, then sweep
int shoot_pass(ShootCtx& X, const ShootPass& ps) {
    mgn_handle* h = X.h; mgn_rollout_desc* d = X.d; mgn_shooting_desc* s = X.s;
    const ShootGroup& G = X.groups[ps.grp];
    const int32_t B = ps.B;
    const int64_t K = G.K;
    const int ns = (int)G.save_step.size();
    mgn_engine* e = h;
    if (B > 1) {
        if (int rc = shoot_companion(h, B, &e)) return rc;
        if (int rc = solver_prepare(e, X.n_grads)) return fail(h, rc, "%s: companion: %s", shoot_who, e->err.c_str());
    }
    auto efail = [&](int rc) { return e == h ? rc : fail(h, rc, "%s: companion: %s", shoot_who, e->err.c_str()); };
    invalidate_static(e);
    X.dw.n_saves = ns;
    X.keep_alive.push_back(std::make_unique<Rollout>(e, &X.dw, G.tg, true, B * X.N, B * X.N));
    Rollout& R = *X.keep_alive.back();
    const size_t nb = (size_t)R.n * 4;
    const size_t eb = tile_floats(e->es[0].ntiles_e, h->cfg.L) * 4;
    Arena ea;
    const int sp = X.tb.active();
    R.tb = &X.tb;
    const SolveWs ws = carve_solve(ea, nb, X.tb.s, X.tb.fsal, true, X.inflow);
    const size_t o_sv = ea.take((size_t)ns * nb), o_el = ea.take(eb), o_tg = ea.take((size_t)ns * nb), o_ct = ea.take(nb), o_a = ea.take(nb),
                 o_yb = ea.take((size_t)(sp - 1) * nb), o_mr = ea.take(X.inflow && B > 1 ? (size_t)B * X.N : 0);
    if ((size_t)(K + 1) > (SIZE_MAX / 8) / (nb > 0 ? nb : 1)) return fail(h, MGN_E_OOM, "%s: %lld stored steps overflow the address space", shoot_who, (long long)K);
    const size_t o_st = ea.take((size_t)sp * K * nb);
    if (int rc = ensure_or_fail(h, e->ode, ea.off, "%s: %.3f GB for a pass of %d windows (stored states and buffers)", shoot_who, (double)ea.off * 1e-9, B))
        return rc;
    char* base = e->ode.as<char>();
    R.bind(base, ws);
    R.frames = X.frl;
    R.mask = X.mkl;
    R.ftab = X.inflow ? X.itd + G.ftab_off + ps.j0 : nullptr;
    R.ftab_ld = (int64_t)G.win.size();
    R.win_rows = X.N;
    R.saves = (float*)(base + o_sv);
    R.partial = nullptr;
    R.elat0_off = o_el;
    uint8_t* mrep = X.inflow ? (B > 1 ? (uint8_t*)(base + o_mr) : X.mkl) : nullptr;
    float* store = (float*)(base + o_st);
    if (e == h) {
        if (int rc = upload_statics(h, d, X.zero_x0.data(), base + o_el, eb)) return rc;
    } else {
        if (int rc = shoot_statics(e, B, X.N, (const float*)(X.sbase + X.o_oh), d->val_mask ? (const float*)(X.sbase + X.o_vm) : nullptr,
                                   (const float*)(X.sbase + X.o_ef), base + o_el, eb)) return efail(rc);
        if (X.inflow) HIPCHK(h, launch_shoot_gather_u8(mrep, X.mkl, (int64_t)B * X.N, X.N, h->stream));
    }
    const int32_t* ix = X.itd + ps.idx_off;
    HIPCHK(h, launch_shoot_gather(R.u, X.gtl, R.n, X.nN, 0, ix, nullptr, 0, h->stream));     // x0 = gt[first[w]]

    // forward: the single-window loop, save points from the group's plan; step i's stage inputs contiguously at steps[i]
    std::vector<float*> steps;
    for (int64_t i = 0; i < K; ++i) steps.push_back(store + (size_t)i * sp * R.n);
    const Rollout::Slot slot = [&](int64_t i, float** out) { *out = steps[i]; return MGN_OK; };
    if (int rc = R.erk_fixed(K, G.save_step, &slot)) return efail(rc);
    if (R.saved != ns) return fail(h, MGN_E_STATE, "%s: %d of %d saves taken", shoot_who, R.saved, ns);
    d->n_accept += (int32_t)(K * B);
    d->n_rhs += R.n_rhs * B;

    // targets of the pass, gathered out of gt on the device
    float* tg = (float*)(base + o_tg);
    float* ctt = (float*)(base + o_ct);
    bool has_ct = false;
    for (int32_t j = 0; j < B; ++j) has_ct = has_ct || G.win[ps.j0 + j] + 1 < s->n_windows;
    HIPCHK(h, launch_shoot_gather(tg, X.gtl, (int64_t)ns * R.n, X.nN, 0, ix + B, nullptr, 0, h->stream));
    if (has_ct) HIPCHK(h, launch_shoot_gather(ctt, X.gtl, R.n, X.nN, 0, ix + B + (size_t)ns * B, nullptr, 0, h->stream));

    SolverSweep S = sweep_setup(R, steps, (float*)(base + o_yb), tg, X.lsd, mrep, has_ct ? ctt : nullptr, (float*)(base + o_a), X.gacc);
    if (e == h) {
        S.onehot = d->node_type_onehot; S.ef_raw = d->ef_raw; S.val_mask = d->val_mask;
    } else {
        S.onehot = X.W1 > 0 ? e->d_nfB.as<float>() : nullptr; S.ef_raw = e->es[0].d_ef.as<float>(); S.val_mask = d->val_mask ? e->d_mask.as<float>() : nullptr;
    }
    S.cw_win = X.cwd + ps.cw_off; S.win_rows = X.N; S.lacc = X.lacc; S.lacc_ld = X.ld; S.lscale = 1.0 / ((double)ns * (double)X.nN);
    if (int rc = erk_sweep(e, S)) return efail(rc);
    if (d->out) {       // the predicted saves in window order
        float* oall = (float*)(X.sbase + X.o_out);
        for (int sv = 0; sv < ns; ++sv)
            for (int32_t j = 0; j < B; ++j)
                HIPCHK(h, hipMemcpyAsync(oall + (size_t)(X.out_row[G.win[ps.j0 + j]] + sv) * X.nN, R.saves + (size_t)sv * R.n + (size_t)j * X.nN,
                                         (size_t)X.nN * 4, hipMemcpyDeviceToDevice, h->stream));
    }
    return MGN_OK;
}

}  // namespace

extern "C" int mgn_shooting_grad(mgn_handle* h, mgn_rollout_desc* d, mgn_shooting_desc* s, const float* gt, const float* loss_scale, float cont_weight,
                                 float* grads, size_t n_grads, float* loss) try {
    const char* who = shoot_who;
    if (!h) return MGN_E_ARG;
    // the arguments first (a host-only handle answers them too)
    if (!d || !s || !gt || !grads || !loss) return fail(h, MGN_E_ARG, "%s: null argument", who);
    if (d->solver != 0 && d->solver != 1) return fail(h, MGN_E_ARG, "%s: solver must be 0 (Euler) or 1 (Tsit5)", who);
    if (d->solver == 1 && s->adaptive != 0)
        return fail(h, MGN_E_UNSUPPORTED, "%s: adaptive Tsit5 windows need a step controller each: call mgn_solver_grad_tsit5 per window", who);
    const int32_t W = s->n_windows;
    if (W < 1 || !s->first || !s->last || !s->t0 || !s->t1) return fail(h, MGN_E_ARG, "%s: needs n_windows >= 1 and first / last / t0 / t1", who);
    if (s->max_windows_per_pass < 0 || s->max_batch_nodes < 0) return fail(h, MGN_E_ARG, "%s: max_windows_per_pass and max_batch_nodes must be >= 0", who);
    for (int32_t w = 0; w < W; ++w)
        if (s->first[w] < 0 || s->last[w] <= s->first[w] || s->last[w] >= s->n_gt)
            return fail(h, MGN_E_ARG, "%s: window %d = (%d, %d) must satisfy 0 <= first < last < n_gt = %d", who, w, s->first[w], s->last[w], s->n_gt);
    s->n_groups = s->n_passes = 0;
    if (int rc = solver_state_checks(h, who)) return rc;
    if (int rc = solver_static_checks(h, d, who)) return rc;
    ShootCtx X(h, d, s, cont_weight, n_grads);
    if (!(X.DG.sdt > 0.0)) return fail(h, MGN_E_ARG, "%s: bad time grid", who);
    if (!(X.DG.dt > 0.0)) return fail(h, MGN_E_ARG, "%s: fixed steps need dt > 0", who);
    if (int rc = solver_inflow_checks(h, d, who, cont_weight)) return rc;
    if (int rc = shoot_plans(X)) return rc;
    if (int rc = solver_prepare(h, n_grads)) return rc;     // fp32, one partition, parameter count; the handle's training state
    s->n_groups = (int32_t)X.groups.size();
    s->n_passes = (int32_t)X.passes.size();
    if (int rc = shoot_stage(X, gt, loss_scale)) return rc;
    d->n_accept = d->n_reject = d->n_rhs = 0;
    for (const ShootPass& ps : X.passes)
        if (int rc = shoot_pass(X, ps)) return rc;
    // results: the gradient finalised once, the loss partials added in a fixed order, one synchronisation
    float* gf = (float*)(X.sbase + X.o_gf);
    HIPCHK(h, launch_grad_finish(X.gacc, gf, (int64_t)h->params.size(), h->stream));
    HIPCHK(h, hipMemcpyAsync(grads, gf, h->params.size() * 4, hipMemcpyDefault, h->stream));
    std::vector<double> lp((size_t)2 * X.ld);
    HIPCHK(h, hipMemcpyAsync(lp.data(), X.lacc, lp.size() * 8, hipMemcpyDeviceToHost, h->stream));
    if (d->out)
        if (int rc = saves_to_caller(h, (const float*)(X.sbase + X.o_out), X.out_row[s->n_windows], d->out)) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    double se = 0.0, sa = 0.0;
    for (int b = 0; b < X.ld; ++b) { se += lp[b]; sa += lp[(size_t)X.ld + b]; }
    *loss = (float)(se + sa);
    return MGN_OK;
} MGN_CATCH(h)
