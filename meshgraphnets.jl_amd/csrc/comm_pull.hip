// k_a2a_pull: the device side of the MGN_COMM_LOCAL transport (comm.cpp: LocalComm).  The RECEIVING rank launches it once per
// collective on its compute stream; it copies every peer's segment straight out of the peer's send buffer into this rank's `recv`.
// It is a copy kernel and nothing else: it polls no memory -- all ordering against the peers is made of HIP events on the host side.
#include "comm.h"

namespace mgn {
namespace {

constexpr int PULL_THREADS = 256;

// One segment: `bytes` (a multiple of 4) from src to dst, both 4-byte aligned.  When src and dst have the same residue mod 16 the body
// moves as 16-byte vectors, lane i at base + 16 i (1 KiB per wave instruction), with a dword loop over the head in front of the first
// 16-byte boundary and over the tail behind the last; otherwise no boundary suits both sides and the whole segment goes by dwords
// (the engine's own segments are whole rows of 128 .. 512 bytes in hipMalloc'ed buffers: always the vector path).
__device__ __forceinline__ void pull_segment(const char* __restrict__ src, char* __restrict__ dst, size_t bytes, size_t t, size_t nt) {
    const size_t ndw = bytes >> 2;
    const uint32_t* s4 = reinterpret_cast<const uint32_t*>(src);
    uint32_t* d4 = reinterpret_cast<uint32_t*>(dst);
    if (((reinterpret_cast<uintptr_t>(src) ^ reinterpret_cast<uintptr_t>(dst)) & 15) != 0) {
        for (size_t i = t; i < ndw; i += nt) d4[i] = s4[i];
        return;
    }
    size_t head = ((16 - (reinterpret_cast<uintptr_t>(dst) & 15)) & 15) >> 2;   // dwords in front of the first 16-byte boundary
    if (head > ndw) head = ndw;
    const size_t nvec = (ndw - head) >> 2;
    const size_t tail0 = head + (nvec << 2);
    if (t < head) d4[t] = s4[t];
    const uint4* sv = reinterpret_cast<const uint4*>(s4 + head);
    uint4* dv = reinterpret_cast<uint4*>(d4 + head);
    for (size_t i = t; i < nvec; i += nt) dv[i] = sv[i];
    if (t < ndw - tail0) d4[tail0 + t] = s4[tail0 + t];                          // (at most 3 dwords each side; nt >= PULL_THREADS)
}

// grid (x, y): the y blocks walk the segments with stride gridDim.y, the x blocks of a row share one segment's bytes
__global__ __launch_bounds__(PULL_THREADS) void k_a2a_pull(const PullTable tab, char* __restrict__ recv) {
    const size_t t = (size_t)blockIdx.x * PULL_THREADS + threadIdx.x, nt = (size_t)gridDim.x * PULL_THREADS;
    for (int s = blockIdx.y; s < tab.n; s += gridDim.y) {
        const PullSeg g = tab.seg[s];
        if (g.bytes == 0) continue;
        pull_segment(static_cast<const char*>(g.src), recv + g.dst_off, g.bytes, t, nt);
    }
}

}  // namespace

hipError_t launch_a2a_pull(const PullTable& tab, void* recv, hipStream_t stream) {
    size_t longest = 0;
    int live = 0;
    for (int s = 0; s < tab.n; ++s) {
        if (tab.seg[s].bytes > longest) longest = tab.seg[s].bytes;
        live += tab.seg[s].bytes != 0;
    }
    if (!live) return hipSuccess;
    // one thread per 16 bytes of the longest segment, at most 64 blocks across it (a halo segment is tens of KiB to a few MiB: the
    // grid-stride loop takes the rest); up to 8 rows of blocks over the segments
    size_t gx = (longest / 16 + PULL_THREADS - 1) / PULL_THREADS;
    gx = gx < 1 ? 1 : (gx > 64 ? 64 : gx);
    const int gy = tab.n < 8 ? tab.n : 8;
    hipLaunchKernelGGL(k_a2a_pull, dim3((unsigned)gx, (unsigned)gy), dim3(PULL_THREADS), 0, stream, tab, static_cast<char*>(recv));
    return hipGetLastError();
}

}  // namespace mgn
