// The launch layer's process-wide state in one place: environment switches, the dynamic-LDS grants of the kernels, the CU count of each
// device.  Handles step from several host threads (mgn_group's rank workers, the thread-rank tests) and may sit on different devices, so
// every piece is atomic or under a mutex, and what belongs to a device is keyed by its ordinal.  The first part is plain C++
// (tests/c_abi/launch_state.cpp compiles it with g++), the second needs hipcc.
#pragma once

#include <atomic>
#include <cstdlib>
#include <map>
#include <mutex>

namespace mgn {

// An environment variable as a number, dflt where it is not set.  WHEN it is read is the caller's choice and part of the variable's
// meaning: at library load (file scope), at first use (function-local static) or at every call.
inline int env_int(const char* name, int dflt) { const char* e = std::getenv(name); return e ? std::atoi(e) : dflt; }
inline double env_double(const char* name, double dflt) { const char* e = std::getenv(name); return e ? std::atof(e) : dflt; }

// A process-wide switch: initial value from the environment, set() behind the mgn_debug_* setters (returns the old value).
// (relaxed atomics: rank threads read while the main thread may set; a switch orders nothing)
class Switch {
    std::atomic<int> v;
public:
    Switch(const char* name, int dflt) : v(env_int(name, dflt)) {}
    operator int() const { return v.load(std::memory_order_relaxed); }
    int set(int x) { return v.exchange(x, std::memory_order_relaxed); }
};

// Bytes of dynamic LDS each kernel has been granted on each device (hipFuncAttributeMaxDynamicSharedMemorySize), from 0: a launch of
// more must raise the grant first.  No HIP call is made here: raise() runs the caller's function under the mutex, so of the threads
// that need the same raise exactly one makes it, and the grant is recorded only where that function returned 0 -- a failed raise is
// tried again by the next launch.
class LdsGrants {
    std::mutex mu;
    std::map<std::pair<int, const void*>, size_t> granted;
public:
    bool need(int dev, const void* kern, size_t lds) {
        std::lock_guard<std::mutex> lock(mu);
        return lds > granted[{dev, kern}];
    }
    template <typename F>
    int raise(int dev, const void* kern, size_t lds, F&& raise_fn) {   // 0: nothing to raise, or raised; else raise_fn()'s error
        std::lock_guard<std::mutex> lock(mu);
        size_t& g = granted[{dev, kern}];
        if (lds <= g) return 0;
        const int e = raise_fn();
        if (e == 0) g = lds;
        return e;
    }
};

// One int per device, asked of query(dev) once
class PerDeviceInt {
    std::mutex mu;
    std::map<int, int> val;
public:
    template <typename F>
    int get(int dev, F&& query) {
        std::lock_guard<std::mutex> lock(mu);
        const auto it = val.find(dev);
        return it != val.end() ? it->second : val[dev] = query(dev);
    }
};

}  // namespace mgn

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

namespace mgn {

inline LdsGrants g_lds_grants;
inline PerDeviceInt g_device_cus;

// CU count of the current device (256 where the runtime does not say)
inline int device_cus() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    return g_device_cus.get(dev, [](int d) {
        hipDeviceProp_t p;
        return hipGetDeviceProperties(&p, d) == hipSuccess && p.multiProcessorCount > 0 ? p.multiProcessorCount : 256;
    });
}

// Every launch with dynamic LDS: the opt-in (needed above 64 KiB) is made once per (device, kernel) and size, off the per-launch path
// -- small meshes are launch-bound.  A failed opt-in is returned and not remembered.
template <typename K, typename A>
hipError_t launch_kernel(K kern, dim3 grid, dim3 block, size_t lds, hipStream_t s, const A& args) {
    const void* fn = reinterpret_cast<const void*>(kern);   // keyed by address: K is only the signature type
    int dev = 0;
    if (const hipError_t e = hipGetDevice(&dev)) return e;
    if (const int e = g_lds_grants.raise(dev, fn, lds, [&] { return (int)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); }))
        return (hipError_t)e;
    hipLaunchKernelGGL(kern, grid, block, lds, s, args);
    return hipGetLastError();
}

}  // namespace mgn
#endif
