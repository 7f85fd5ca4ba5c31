// The host-only planning of csrc/mgn_solve.cpp: fixed_grid, the frame plan of mgn_shooting_grad (erk_eval_times) and carve_solve's sizes.
// The program takes mgn_solve.cpp into its own translation unit (the pieces live in its unnamed namespace) and calls nothing that launches,
// allocates on a device or needs the rest of the library: the drivers it does not call are discarded at link time, it needs neither the
// library nor a GPU.
//   g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I<rocm>/include -I include -ffunction-sections -fdata-sections solve_plan.cpp \
//       -Wl,--gc-sections -o solve_plan && ./solve_plan      (prints "solve_plan OK"; add -fsanitize=address,undefined for a checked run)
// Every check() that fails prints its line; the exit status is the number of failures.
#include <cstdio>
#include <vector>

#include "../../meshgraphnets.jl_amd/csrc/mgn_solve.cpp"

// the one function of the library the planning calls: it formats a refusal
int mgn::fail(mgn_engine*, int code, const char*, ...) { return code; }

static int g_failures = 0;
#define check(COND)                                                                \
    do {                                                                           \
        if (!(COND)) {                                                             \
            std::fprintf(stderr, "line %d: check failed: %s\n", __LINE__, #COND);  \
            ++g_failures;                                                          \
        }                                                                          \
    } while (0)

// The loops mgn_shooting_grad's frame table was written with before it walked the tableau: Euler one evaluation at t per step; Tsit5 k1
// once, then stages 2 .. 6 at c_i and stage 7 at t_{n+1}
static const double OLD_TS_C[7] = {0.0, 0.161, 0.327, 0.9, 0.9800255409045097, 1.0, 1.0};
static std::vector<double> old_times(bool euler, const TimeGrid& T, int64_t K) {
    std::vector<double> out;
    double t = T.t0;
    if (!euler) out.push_back(t);
    for (int64_t i = 0; i < K; ++i) {
        const double tn = T.next(i, K, t);
        if (euler) {
            out.push_back(t);
        } else {
            for (int sidx = 1; sidx < 6; ++sidx) out.push_back(T.tt(t + T.tt(OLD_TS_C[sidx] * T.dt)));
            out.push_back(tn);
        }
        t = tn;
    }
    return out;
}

static mgn_rollout_desc desc(int time_f64, int K, double t0) {
    mgn_rollout_desc d{};
    d.time_f64 = time_f64;
    d.t0 = (float)t0; d.dt = 0.01f; d.saves_dt = 0.01f; d.t1 = (float)(t0 + K * 0.01);
    d.t0_f64 = t0; d.dt_f64 = 0.01; d.saves_dt_f64 = 0.01; d.t1_f64 = t0 + K * 0.01;
    d.n_saves = K + 1;
    return d;
}

int main() {
    for (int f64 = 0; f64 < 2; ++f64)
        for (int K : {1, 3})
            for (double t0 : {0.0, 0.37}) {
                const mgn_rollout_desc d = desc(f64, K, t0);
                const TimeGrid T(&d);
                int64_t Kg = -1;
                std::vector<int64_t> plan;
                check(fixed_grid(nullptr, "solve_plan", T, d.n_saves, &Kg, plan) == MGN_OK);
                check(Kg == K && (int)plan.size() == K + 1);
                for (int i = 0; i <= K && i < (int)plan.size(); ++i) check(plan[i] == i);
                for (bool euler : {true, false}) {
                    const Erk& tb = euler ? erk_euler() : erk_tsit5();
                    std::vector<double> got;
                    check(erk_eval_times(tb, T, K, [&](double t) { got.push_back(t); return MGN_OK; }) == MGN_OK);
                    const std::vector<double> want = old_times(euler, T, K);
                    check(got.size() == (size_t)(euler ? K : 1 + 6 * K));
                    check(got.size() == want.size());
                    for (size_t i = 0; i < got.size() && i < want.size(); ++i) check(got[i] == want[i]);
                }
                // a save beyond the end of the solve is refused
                check(fixed_grid(nullptr, "solve_plan", T, d.n_saves + 1, &Kg, plan) == MGN_E_ARG);
            }
    check(erk_euler().s == 1 && erk_euler().active() == 1 && !erk_euler().fsal && erk_euler().b[0] == 1.0 && erk_euler().c[0] == 0.0);
    check(erk_tsit5().s == 7 && erk_tsit5().active() == 6 && erk_tsit5().fsal);
    for (int i = 0; i < 7; ++i) check(erk_tsit5().c[i] == OLD_TS_C[i]);

    // carve_solve: every array the method has is 256-byte aligned and overlaps no other; one stage takes one k and neither utmp nor zs
    const size_t nb = 1000 * 2 * 4 + 4;      // (no multiple of 256)
    for (int s : {1, 7})
        for (int fixed = 0; fixed < 2; ++fixed)
            for (int zc = 0; zc < 2; ++zc) {
                const bool fsal = s == 7;
                Arena a;
                a.take(12);
                const SolveWs w = carve_solve(a, nb, s, fsal, fixed != 0, zc != 0);
                std::vector<size_t> offs{w.u};
                if (w.has_un) offs.push_back(w.un);
                if (s > 1) offs.push_back(w.ut);
                for (int j = 0; j < s; ++j) offs.push_back(w.k[j]);
                if (zc) offs.push_back(w.za);
                if (zc && s > 1) offs.push_back(w.zs);
                if (w.has_z7) offs.push_back(w.z7);
                check(w.has_un == (fsal || !fixed) && w.has_z7 == (zc && fsal));
                check(offs.size() == (size_t)(1 + (w.has_un ? 1 : 0) + (s > 1 ? 1 : 0) + s + (zc ? (s > 1 ? 2 : 1) + (fsal ? 1 : 0) : 0)));
                for (size_t i = 0; i < offs.size(); ++i) {
                    check(offs[i] % 256 == 0 && offs[i] >= 256 && offs[i] + nb <= a.off);
                    for (size_t j = 0; j < i; ++j) check(offs[i] >= offs[j] + nb || offs[j] >= offs[i] + nb);
                }
                check(a.off == 256 + offs.size() * ((nb + 255) & ~(size_t)255));
            }
    if (g_failures == 0) std::printf("solve_plan OK\n");
    return g_failures;
}
