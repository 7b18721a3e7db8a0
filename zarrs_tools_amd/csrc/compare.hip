// compare.hip — the per-element work of zarrs_validate (src/bin/zarrs_validate.rs:145-147,
// `bytes_first == bytes_second`): two contiguous runs a and b of n elements of one data type,
// compared by their storage bits. A NaN equals a NaN with the same bits and differs from one with
// another payload, +0.0 differs from -0.0, bool is a byte: the element's size is all that
// matters, so there are four instantiations (1, 2, 4 and 8 bytes).
//
// Both runs are read as info.hip reads one (zt_info.hpp): a decides head, vectors and tail. When
// b is congruent to a mod 16 its vectors are aligned 16-byte loads too; otherwise b is loaded
// with the alignment it has (a 16-byte copy from an element-aligned pointer). A lane XORs the four
// words of each pair of vectors; when a wave ballot finds no nonzero word in any lane of a step
// (equal arrays, the common case) nothing more happens in that step. Otherwise the lane counts
// the elements (not the words or bytes) that differ and keeps the smallest differing index
// (base + the run-local index, so a caller that folds an array run by run gets the C-order
// index in the whole array). Lanes reduce with cross-lane shuffles, waves through LDS, and one
// lane of a workgroup that saw a difference folds (count, index) into the two-word device state
// with a 64-bit integer atomic add and atomic min. Integer add and min commute: the result does
// not depend on the launch geometry. The state starts as (0, all ones) = "equal".
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "zt_info.hpp"
#include "zt_kernels.hpp"

namespace zt {

namespace {

template <int ESZ> struct UintOf;
template <> struct UintOf<1> { using type = uint8_t; };
template <> struct UintOf<2> { using type = uint16_t; };
template <> struct UintOf<4> { using type = uint32_t; };
template <> struct UintOf<8> { using type = uint64_t; };

constexpr unsigned long long kNone = ~0ull;

// The elements of ESZ bytes that are nonzero in the XOR x of two vectors: how many, and the
// index within the vector of the first (PER if none).
template <int ESZ>
__device__ __forceinline__ void differing(const uint32_t (&x)[4], int& count, int& first) {
    count = 0;
    first = 16 / ESZ;
    if constexpr (ESZ == 8) {
#pragma unroll
        for (int i = 1; i >= 0; --i)
            if (x[2 * i] | x[2 * i + 1]) {
                ++count;
                first = i;
            }
    } else if constexpr (ESZ == 4) {
#pragma unroll
        for (int i = 3; i >= 0; --i)
            if (x[i]) {
                ++count;
                first = i;
            }
    } else {
        // the top bit of every element of the word that is nonzero
        constexpr uint32_t kLow = ESZ == 2 ? 0x7FFF7FFFu : 0x7F7F7F7Fu;
        constexpr int kShift = ESZ == 2 ? 4 : 3;  // log2 of the element's bits
        constexpr int kPerWord = 4 / ESZ;
#pragma unroll
        for (int i = 3; i >= 0; --i) {
            const uint32_t m = (x[i] | ((x[i] & kLow) + kLow)) & ~kLow;
            if (m) {
                count += __builtin_popcount(m);
                first = i * kPerWord + (__builtin_ctz(m) >> kShift);
            }
        }
    }
}

__global__ void compare_init_kernel(unsigned long long* state) {
    state[0] = 0ull;
    state[1] = kNone;
}

// ALIGNED: b + head lies on a 16-byte boundary as a + head does
template <int ESZ, bool ALIGNED>
__global__ __launch_bounds__(kInfoThreads) void compare_kernel(
    const typename UintOf<ESZ>::type* a, const typename UintOf<ESZ>::type* b, int64_t n, int head,
    int64_t nvec, unsigned long long base, unsigned long long* state) {
    using U = typename UintOf<ESZ>::type;
    constexpr int PER = 16 / ESZ;
    unsigned long long count = 0, first = kNone;
    const Vec16A* va = reinterpret_cast<const Vec16A*>(a + head);
    const U* eb = b + head;
    const int64_t steps = (nvec + kInfoStepVecs - 1) / kInfoStepVecs;
    for (int64_t s = blockIdx.x; s < steps; s += gridDim.x) {
        const int64_t v0 = s * kInfoStepVecs + threadIdx.x;
        Vec16A qa[kInfoUnroll] = {}, qb[kInfoUnroll] = {};  // a lane past the end: 0 ^ 0
#pragma unroll
        for (int u = 0; u < kInfoUnroll; ++u) {
            const int64_t v = v0 + (int64_t)u * kInfoThreads;
            if (v < nvec) {
                qa[u] = va[v];
                if constexpr (ALIGNED) qb[u] = reinterpret_cast<const Vec16A*>(eb)[v];
                else __builtin_memcpy(&qb[u], eb + v * PER, 16);
            }
        }
        uint32_t x[kInfoUnroll][4], any = 0;
#pragma unroll
        for (int u = 0; u < kInfoUnroll; ++u) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                x[u][i] = qa[u].w[i] ^ qb[u].w[i];
                any |= x[u][i];
            }
        }
        if (__builtin_amdgcn_ballot_w64(any != 0) == 0) continue;  // the wave's vectors are equal
#pragma unroll
        for (int u = kInfoUnroll - 1; u >= 0; --u) {  // downwards: `first` ends at the smallest
            int c, f;
            differing<ESZ>(x[u], c, f);
            if (c) {
                count += (unsigned)c;
                const unsigned long long idx =
                    base + (unsigned long long)head +
                    (unsigned long long)(v0 + (int64_t)u * kInfoThreads) * PER + (unsigned)f;
                first = idx < first ? idx : first;
            }
        }
    }
    if (blockIdx.x == 0) {  // head and tail: fewer than one vector each
        const int64_t t0 = head + nvec * PER;
        if ((int)threadIdx.x < head && a[threadIdx.x] != b[threadIdx.x]) {
            ++count;
            const unsigned long long idx = base + threadIdx.x;
            first = idx < first ? idx : first;
        }
        if (t0 + threadIdx.x < n && a[t0 + threadIdx.x] != b[t0 + threadIdx.x]) {
            ++count;
            const unsigned long long idx = base + (unsigned long long)(t0 + threadIdx.x);
            first = idx < first ? idx : first;
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned long long oc = shfl_xor_key(count, m), of = shfl_xor_key(first, m);
        count += oc;
        first = of < first ? of : first;
    }
    __shared__ unsigned long long wcount[kInfoThreads / 64], wfirst[kInfoThreads / 64];
    if ((threadIdx.x & 63) == 0) {
        wcount[threadIdx.x >> 6] = count;
        wfirst[threadIdx.x >> 6] = first;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < kInfoThreads / 64; ++w) {
            count += wcount[w];
            first = wfirst[w] < first ? wfirst[w] : first;
        }
        if (count) {  // this workgroup saw a difference
            atomicAdd(&state[0], count);
            atomicMin(&state[1], first);
        }
    }
}

template <int ESZ, bool ALIGNED>
hipError_t launch_compare_t(const void* a, const void* b, int64_t n, int64_t base, void* state,
                            hipStream_t s) {
    using U = typename UintOf<ESZ>::type;
    int head;
    int64_t nvec;
    static const int resident = resident_blocks(compare_kernel<ESZ, ALIGNED>);  // asked once
    const unsigned grid = split_run(resident, a, n, ESZ, &head, &nvec);
    hipLaunchKernelGGL((compare_kernel<ESZ, ALIGNED>), dim3(grid), dim3(kInfoThreads), 0, s,
                       static_cast<const U*>(a), static_cast<const U*>(b), n, head, nvec,
                       (unsigned long long)base, static_cast<unsigned long long*>(state));
    return hipGetLastError();
}

template <int ESZ>
hipError_t launch_compare_e(const void* a, const void* b, int64_t n, int64_t base, void* state,
                            hipStream_t s) {
    if ((((uintptr_t)a ^ (uintptr_t)b) & 15) == 0)
        return launch_compare_t<ESZ, true>(a, b, n, base, state, s);
    return launch_compare_t<ESZ, false>(a, b, n, base, state, s);
}

}  // namespace

hipError_t launch_compare_init(void* state, hipStream_t s) {
    hipLaunchKernelGGL(compare_init_kernel, dim3(1), dim3(1), 0, s,
                       static_cast<unsigned long long*>(state));
    return hipGetLastError();
}

hipError_t launch_compare_accumulate(const void* a, const void* b, int esz, int64_t n,
                                     int64_t base, void* state, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    switch (esz) {
    case 1: return launch_compare_e<1>(a, b, n, base, state, s);
    case 2: return launch_compare_e<2>(a, b, n, base, state, s);
    case 4: return launch_compare_e<4>(a, b, n, base, state, s);
    case 8: return launch_compare_e<8>(a, b, n, base, state, s);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace zt
