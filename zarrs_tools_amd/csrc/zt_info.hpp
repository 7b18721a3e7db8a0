// zt_info.hpp — how the whole-array reductions (info.hip: range, histogram; compare.hip: the
// bitwise comparison) read a contiguous run of n elements at element alignment: the elements
// before the first 16-byte boundary (the head) and those after the last whole 16-byte vector (the
// tail) one per lane by workgroup 0, the vectors in between as aligned 16-byte loads, kInfoUnroll
// per lane and step, a step being kInfoThreads * kInfoUnroll consecutive vectors (16 KiB). Steps
// are grid-strided over at most one resident round of workgroups (info_max_blocks()).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "zt_kernels.hpp"

namespace zt {

constexpr int kInfoThreads = 256;
constexpr int kInfoUnroll = 4;  // 16-byte vectors a lane loads per step
constexpr int64_t kInfoStepVecs = (int64_t)kInfoThreads * kInfoUnroll;

struct __attribute__((aligned(16))) Vec16A {
    uint32_t w[4];
};

template <typename K>
__device__ __forceinline__ K shfl_xor_key(K v, int m) {
    if constexpr (sizeof(K) == 4) {
        return (K)__shfl_xor((unsigned)v, m, 64);
    } else {
        const unsigned lo = __shfl_xor((unsigned)v, m, 64);
        const unsigned hi = __shfl_xor((unsigned)(v >> 32), m, 64);
        return ((K)hi << 32) | lo;
    }
}

// The most workgroups of a kernel the device holds at once (0 if the runtime cannot tell).
template <typename K>
int resident_blocks(K kernel) {
    int dev = 0, cus = 0, per_cu = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kInfoThreads, 0) !=
            hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return cus * per_cu;
}

// head elements, whole vectors and the grid of a run of n elements of `esz` bytes at p
inline unsigned split_run(int resident, const void* p, int64_t n, int esz, int* head,
                          int64_t* nvec) {
    const int per = 16 / esz;
    int64_t h = (int64_t)((16 - ((uintptr_t)p & 15)) & 15) / esz;
    if (h > n) h = n;
    *head = (int)h;
    *nvec = (n - h) / per;
    const int64_t steps = (*nvec + kInfoStepVecs - 1) / kInfoStepVecs;
    int64_t cap = info_max_blocks();
    if (resident > 0 && resident < cap) cap = resident;
    return (unsigned)(steps < 1 ? 1 : steps < cap ? steps : cap);
}

}  // namespace zt
