// The plain C++ part of csrc/launch.hpp (no HIP) and tfrecord.cpp's CRC-32C under eight threads.
//   g++ -std=c++17 -pthread launch_state.cpp -o launch_state && ./launch_state      (prints "launch_state OK")
// Every check() that fails prints its line; the exit status is the number of failures.
#include <algorithm>
#include <condition_variable>
#include <cstdio>
#include <thread>
#include <vector>

#include "../../meshgraphnets.jl_amd/csrc/launch.hpp"
#include "../../meshgraphnets.jl_amd/csrc/tfrecord.cpp"   // crc32c (its unnamed namespace)

using namespace mgn;

static std::atomic<int> g_failures{0};
#define check(COND)                                                                \
    do {                                                                           \
        if (!(COND)) {                                                             \
            std::fprintf(stderr, "line %d: check failed: %s\n", __LINE__, #COND);  \
            g_failures.fetch_add(1);                                               \
        }                                                                          \
    } while (0)

constexpr int NTHREADS = 8;

class Barrier {
    std::mutex mu;
    std::condition_variable cv;
    int waiting = 0, generation = 0;
public:
    void wait() {
        std::unique_lock<std::mutex> lock(mu);
        const int gen = generation;
        if (++waiting == NTHREADS) {
            waiting = 0;
            ++generation;
            cv.notify_all();
        } else {
            cv.wait(lock, [&] { return generation != gen; });
        }
    }
};

template <typename F>
static void on_threads(F&& body) {
    std::vector<std::thread> th;
    for (int t = 0; t < NTHREADS; ++t) th.emplace_back([&body, t] { body(t); });
    for (std::thread& x : th) x.join();
}

static const char g_kernels[3] = {};   // three addresses to stand for kernels
constexpr int NDEV = 2, NKERN = 3, NSIZE = 4;
static const size_t g_sizes[NSIZE] = {4096, 64 * 1024 + 64, 150 * 1024, 160 * 1024};   // ascending: each exceeds every grant before it

static void grants_one_thread() {
    LdsGrants g;
    const void* k = &g_kernels[0];
    int calls = 0;
    const auto ok = [&] { ++calls; return 0; };
    check(g.need(0, k, 1));                            // the grant starts at 0
    check(!g.need(0, k, 0));
    check(g.raise(0, k, 1000, ok) == 0 && calls == 1);
    check(!g.need(0, k, 1000) && !g.need(0, k, 999) && g.need(0, k, 1001));
    check(g.raise(0, k, 500, ok) == 0 && calls == 1);  // below the grant: nothing to raise, and the grant stays
    check(!g.need(0, k, 1000) && g.need(0, k, 1001));
    check(g.raise(0, k, 2000, ok) == 0 && calls == 2);
    check(!g.need(0, k, 2000) && g.need(0, k, 2001));
    // another device, the same kernel: its own grant
    check(g.need(1, k, 1));
    check(g.raise(1, k, 300, ok) == 0 && calls == 3);
    check(!g.need(1, k, 300) && g.need(1, k, 301) && !g.need(0, k, 2000));
    // another kernel on the same device as well
    check(g.need(0, &g_kernels[1], 1));
    // a failed raise is returned and leaves no grant behind: the next launch asks again
    int failed = 0;
    const auto fail = [&] { ++failed; return 7; };
    check(g.raise(0, k, 3000, fail) == 7 && failed == 1);
    check(g.need(0, k, 3000) && !g.need(0, k, 2000));
    check(g.raise(0, k, 3000, fail) == 7 && failed == 2);
    check(g.raise(0, k, 3000, ok) == 0 && calls == 4 && !g.need(0, k, 3000));
    check(g.raise(2, k, 100, fail) == 7 && g.need(2, k, 1));   // (a pair that never had a grant)
}

static void grants_eight_threads() {
    LdsGrants g;
    Barrier bar;
    std::atomic<int> raised[NDEV][NKERN][NSIZE] = {}, failed{0};
    on_threads([&](int t) {
        for (int si = 0; si < NSIZE; ++si) {
            const auto each_pair = [&](auto&& f) {
                for (int i = 0; i < NDEV * NKERN; ++i) f(((i + t) % (NDEV * NKERN)) / NKERN, ((i + t) % (NDEV * NKERN)) % NKERN);   // every thread starts at another pair
            };
            bar.wait();   // all eight ask for the same size at once
            if (si == 2) {   // first raises that fail: every thread that asks is told to raise, and none leaves a grant
                each_pair([&](int dev, int kern) { check(g.raise(dev, &g_kernels[kern], g_sizes[si], [&] { failed.fetch_add(1); return 1; }) == 1); });
                bar.wait();
            }
            each_pair([&](int dev, int kern) {
                check(g.raise(dev, &g_kernels[kern], g_sizes[si], [&] { raised[dev][kern][si].fetch_add(1); return 0; }) == 0);
                check(!g.need(dev, &g_kernels[kern], g_sizes[si]));
            });
        }
    });
    for (int dev = 0; dev < NDEV; ++dev)
        for (int kern = 0; kern < NKERN; ++kern) {
            for (int si = 0; si < NSIZE; ++si) check(raised[dev][kern][si].load() == 1);   // exactly one thread raised, whatever the interleaving
            check(!g.need(dev, &g_kernels[kern], g_sizes[NSIZE - 1]) && g.need(dev, &g_kernels[kern], g_sizes[NSIZE - 1] + 1));
        }
    check(failed.load() == NTHREADS * NDEV * NKERN);
}

static void switches() {
    setenv("MGN_TEST_LAUNCH_STATE", "5", 1);
    Switch from_env{"MGN_TEST_LAUNCH_STATE", 1};
    unsetenv("MGN_TEST_LAUNCH_STATE");
    Switch dflt{"MGN_TEST_LAUNCH_STATE", 1};
    check(from_env == 5 && dflt == 1);
    check(env_int("MGN_TEST_LAUNCH_STATE", -3) == -3 && env_double("MGN_TEST_LAUNCH_STATE", 2.5) == 2.5);
    setenv("MGN_TEST_LAUNCH_STATE", "0.25", 1);
    check(env_double("MGN_TEST_LAUNCH_STATE", 2.5) == 0.25 && env_int("MGN_TEST_LAUNCH_STATE", 9) == 0);
    unsetenv("MGN_TEST_LAUNCH_STATE");
    check(dflt.set(4) == 1 && dflt == 4 && dflt.set(0) == 4 && dflt == 0);
    // set() is one exchange: over all threads the values handed back, with the one left in the switch, are the values put in
    constexpr int PER = 1000;
    std::vector<int> got[NTHREADS];
    on_threads([&](int t) {
        for (int i = 0; i < PER; ++i) {
            got[t].push_back(dflt.set(1 + t * PER + i));
            (void)(int)dflt;
        }
    });
    std::vector<int> all{(int)dflt};
    for (const std::vector<int>& v : got) all.insert(all.end(), v.begin(), v.end());
    std::sort(all.begin(), all.end());
    check((int)all.size() == NTHREADS * PER + 1);
    for (int i = 0; i < (int)all.size(); ++i) check(all[i] == i);
}

static void per_device_int() {
    PerDeviceInt cache;
    Barrier bar;
    constexpr int DEVS = 4;
    std::atomic<int> queries[DEVS] = {};
    on_threads([&](int t) {
        bar.wait();
        for (int i = 0; i < 1000; ++i) {
            const int dev = (i + t) % DEVS;
            check(cache.get(dev, [&](int d) { queries[d].fetch_add(1); return 100 + d; }) == 100 + dev);
        }
    });
    for (int d = 0; d < DEVS; ++d) check(queries[d].load() == 1);
}

static void crc_first_call() {
    const char* msg = "123456789";
    std::vector<uint8_t> buf(4099);
    for (size_t i = 0; i < buf.size(); ++i) buf[i] = (uint8_t)(i * 131 + 7);
    Barrier bar;
    uint32_t small[NTHREADS], big[NTHREADS];
    on_threads([&](int t) {
        bar.wait();   // the first crc32c call of the process, from all eight threads at once: the table is built under them
        big[t] = crc32c(buf.data(), buf.size());
        small[t] = crc32c(reinterpret_cast<const uint8_t*>(msg), 9);
    });
    for (int t = 0; t < NTHREADS; ++t) check(small[t] == 0xE3069283u && big[t] == big[0]);   // CRC-32C check value
}

int main() {
    crc_first_call();
    grants_one_thread();
    grants_eight_threads();
    switches();
    per_device_int();
    if (g_failures.load() == 0) std::puts("launch_state OK");
    return g_failures.load() > 255 ? 255 : g_failures.load();
}
