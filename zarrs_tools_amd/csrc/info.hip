// info.hip — the whole-array reductions of zarrs_info: `range` (src/info/range.rs) and
// `histogram` (src/info/histogram.rs), on a contiguous run of n elements.
//
// Both kernels read the run the same way (zt_info.hpp, shared with compare.hip). The run needs
// element alignment only (a device view may
// start anywhere): the elements before the first 16-byte boundary (the head) and those after the
// last whole 16-byte vector (the tail) are read one per lane by workgroup 0; the vectors in
// between are read as aligned 16-byte loads, kInfoUnroll per lane and step, a step being
// kInfoThreads * kInfoUnroll consecutive vectors (16 KiB). Steps are grid-strided over at most
// one resident round of workgroups (info_max_blocks()).
//
// Range: each lane keeps the smallest and largest orderable key of its non-NaN elements (unsigned:
// the value; signed: the sign bit flipped; floats: the bits with the sign bit set when positive
// and all bits flipped when negative, so -0.0 < +0.0 and -inf / +inf are the extremes). Lanes
// reduce with cross-lane shuffles, waves through LDS, and one lane folds the workgroup's pair
// into the two-word device state with 64-bit integer atomic min / max. Integer min / max commute:
// the result does not depend on the launch geometry. The state starts as (all ones, 0); no
// element can leave min > max, so that is "none".
//
// Histogram: bin = min(floor(max((x as f64 - min) / (max - min) * n_bins, 0)) as usize, n_bins - 1)
// (histogram.rs:51-68) in f64, one rounding per operation (-ffp-contract=off, IEEE division).
// 8-bit types look the bin up in a 256-entry LDS table each workgroup builds with that formula.
// Up to kInfoLdsBins bins: u32 bins private to the workgroup in LDS, R = 2^k replicas of each
// (bin * R + lane % R: lanes that hold one bin fall on R different banks), flushed with 64-bit
// integer atomic adds to the u64 histogram. More bins: lanes add to the u64 histogram directly.
// When every element of a wave's vectors falls in one bin (a constant background), one lane adds
// the count instead of every lane adding 1 per element. Otherwise lanes add 1 per element where
// a bin has 8 or more replicas; with fewer, and on global bins, element by element the lanes
// that share the first active lane's bin add their count once, and so do, among the lanes left,
// those that share the first of them's (a background that fills most of a wave costs one add,
// not one serialised add per lane, unless neither of the two leading lanes lies in it).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdlib>
#include <limits>
#include <type_traits>

#include "zt_device.hpp"
#include "zt_info.hpp"
#include "zt_kernels.hpp"

namespace zt {

namespace {

// A workgroup flushes its LDS bins after this many steps: at most 2^17 steps * 2^10 vectors * 16
// elements = 2^31 elements (plus < 32 of head and tail) between flushes, so a u32 bin cannot wrap.
constexpr int kInfoFlushSteps = 1 << 17;

// ---- range ---------------------------------------------------------------------------------------

template <typename T> struct KeyOf { using type = uint32_t; };
template <> struct KeyOf<int64_t> { using type = uint64_t; };
template <> struct KeyOf<uint64_t> { using type = uint64_t; };
template <> struct KeyOf<double> { using type = uint64_t; };

// the orderable key of x; false for a NaN (ignored, as PartialOrd makes it: range.rs:115-116)
template <typename T>
__device__ __forceinline__ bool range_key(T x, typename KeyOf<T>::type& k) {
    if constexpr (std::is_same_v<T, float>) {
        const uint32_t b = f2u(x);
        k = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
        return (b & 0x7FFFFFFFu) <= 0x7F800000u;
    } else if constexpr (std::is_same_v<T, double>) {
        const uint64_t b = d2u(x);
        k = (b >> 63) ? ~b : (b | 0x8000000000000000ull);
        return (b & 0x7FFFFFFFFFFFFFFFull) <= 0x7FF0000000000000ull;
    } else if constexpr (std::is_same_v<T, f16_t>) {
        const uint32_t b = x.bits;
        k = (b & 0x8000u) ? (~b & 0xFFFFu) : (b | 0x8000u);
        return (b & 0x7FFFu) <= 0x7C00u;
    } else if constexpr (std::is_same_v<T, bf16_t>) {
        const uint32_t b = x.bits;
        k = (b & 0x8000u) ? (~b & 0xFFFFu) : (b | 0x8000u);
        return (b & 0x7FFFu) <= 0x7F80u;
    } else if constexpr (std::is_signed_v<T>) {
        using K = typename KeyOf<T>::type;
        using U = std::make_unsigned_t<T>;
        k = (K)(U)(x ^ std::numeric_limits<T>::min());
        return true;
    } else {
        k = x;
        return true;
    }
}

__global__ void range_init_kernel(unsigned long long* state) {
    state[0] = ~0ull;
    state[1] = 0ull;
}

template <typename T>
__global__ __launch_bounds__(kInfoThreads) void range_kernel(const T* p, int64_t n, int head,
                                                             int64_t nvec,
                                                             unsigned long long* state) {
    using K = typename KeyOf<T>::type;
    constexpr int PER = 16 / (int)sizeof(T);
    K lo = ~(K)0, hi = 0;
    auto take = [&](T x) {
        K k;
        if (range_key<T>(x, k)) {
            lo = k < lo ? k : lo;
            hi = k > hi ? k : hi;
        }
    };
    const Vec16A* body = reinterpret_cast<const Vec16A*>(p + head);
    const int64_t steps = (nvec + kInfoStepVecs - 1) / kInfoStepVecs;
    for (int64_t s = blockIdx.x; s < steps; s += gridDim.x) {
        const int64_t v0 = s * kInfoStepVecs + threadIdx.x;
        Vec16A q[kInfoUnroll];
#pragma unroll
        for (int u = 0; u < kInfoUnroll; ++u) {
            const int64_t v = v0 + (int64_t)u * kInfoThreads;
            // (a lane past the end takes its first vector again: no effect on a min / max)
            q[u] = body[v < nvec ? v : v0 < nvec ? v0 : 0];
        }
#pragma unroll
        for (int u = 0; u < kInfoUnroll; ++u) {
            T e[PER];
            __builtin_memcpy(e, &q[u], 16);
            if (v0 < nvec) {
#pragma unroll
                for (int i = 0; i < PER; ++i) take(e[i]);
            }
        }
    }
    if (blockIdx.x == 0) {  // head and tail: fewer than one vector each
        const int64_t t0 = head + nvec * PER;
        if ((int)threadIdx.x < head) take(p[threadIdx.x]);
        if (t0 + threadIdx.x < n) take(p[t0 + threadIdx.x]);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const K ol = shfl_xor_key(lo, m), oh = shfl_xor_key(hi, m);
        lo = ol < lo ? ol : lo;
        hi = oh > hi ? oh : hi;
    }
    __shared__ K wlo[kInfoThreads / 64], whi[kInfoThreads / 64];
    if ((threadIdx.x & 63) == 0) {
        wlo[threadIdx.x >> 6] = lo;
        whi[threadIdx.x >> 6] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < kInfoThreads / 64; ++w) {
            lo = wlo[w] < lo ? wlo[w] : lo;
            hi = whi[w] > hi ? whi[w] : hi;
        }
        if (lo <= hi) {  // this workgroup saw a non-NaN element
            atomicMin(&state[0], (unsigned long long)lo);
            atomicMax(&state[1], (unsigned long long)hi);
        }
    }
}

// ---- histogram -----------------------------------------------------------------------------------

struct HistArgs {
    double mn, range, nb;  // min, max - min (one rounding), n_bins as f64
    uint32_t last;         // n_bins - 1
    int32_t log2_r;        // LDS form: replicas per bin = 1 << log2_r
    int64_t n_bins;
};

template <typename T>
__device__ __forceinline__ uint32_t bin_of(T x, const HistArgs& a) {
    const double norm = (Elem<T>::to_f64(x) - a.mn) / a.range;
    double s = norm * a.nb;
    s = s > 0.0 ? s : 0.0;  // f64::max(s, 0.0): NaN and negatives -> 0
    s = __builtin_floor(s);
    return s >= (double)a.last ? a.last : (uint32_t)s;  // `as usize` saturates; min(n_bins - 1)
}

template <typename T, bool LDS>
__global__ __launch_bounds__(kInfoThreads) void hist_kernel(const T* p, int64_t n, int head,
                                                            int64_t nvec, const HistArgs a,
                                                            unsigned long long* hist) {
    constexpr int PER = 16 / (int)sizeof(T);
    constexpr bool kTable = sizeof(T) == 1;
    __shared__ uint32_t bins[LDS ? kInfoLdsBins : 1];
    __shared__ uint32_t table[kTable ? 256 : 1];
    const int lane = threadIdx.x & 63;
    const uint32_t rep = LDS ? (uint32_t)lane & ((1u << a.log2_r) - 1u) : 0u;
    if constexpr (LDS) {
        for (int i = threadIdx.x; i < kInfoLdsBins; i += kInfoThreads) bins[i] = 0;
    }
    if constexpr (kTable) {
        T x;
        const uint8_t byte = (uint8_t)threadIdx.x;
        __builtin_memcpy(&x, &byte, 1);
        table[threadIdx.x] = bin_of<T>(x, a);
    }
    if constexpr (LDS || kTable) __syncthreads();
    auto bin = [&](T x) -> uint32_t {
        if constexpr (kTable) {
            uint8_t byte;
            __builtin_memcpy(&byte, &x, 1);
            return table[byte];
        } else {
            return bin_of<T>(x, a);
        }
    };
    auto add = [&](uint32_t b, uint32_t count) {
        if constexpr (LDS) atomicAdd(&bins[(b << a.log2_r) + rep], count);
        else atomicAdd(&hist[b], (unsigned long long)count);
    };
    // Global bins: the wave's last group (bin, count) waits here and grows while the groups that
    // follow fall in the same bin, so a background costs one atomic per run of groups, not one
    // per group on a single address. Called by every active lane of the wave; lanes only ever
    // leave the loop below for good, lowest vectors last, so lane 0's copy is always current.
    uint32_t pend_bin = 0, pend_count = 0;
    auto add_group = [&](uint32_t b, uint32_t count, bool leader) {
        if constexpr (LDS) {
            if (leader) add(b, count);
        } else {
            if (b == pend_bin && pend_count < 0x80000000u) {
                pend_count += count;
            } else {
                if (leader && pend_count) add(pend_bin, pend_count);
                pend_bin = b;
                pend_count = count;
            }
        }
    };
    auto flush = [&]() {
        if constexpr (LDS) {
            __syncthreads();
            const int r = 1 << a.log2_r;
            for (int b = threadIdx.x; b < (int)a.n_bins; b += kInfoThreads) {
                uint32_t sum = 0;
                for (int i = 0; i < r; ++i) {
                    sum += bins[b * r + i];
                    bins[b * r + i] = 0;
                }
                if (sum) atomicAdd(&hist[b], (unsigned long long)sum);
            }
            __syncthreads();
        }
    };
    // The leader rounds below cost about a third more time on noise (1.34 against 0.99 ms for
    // 2^30 f32 elements) and pay where a bin that most lanes share has few addresses: without
    // them a volume that is 90 % one value takes 3.2 ms at 4096 bins (one replica) and 11.6 s on
    // global bins. 8 replicas or more spread such a bin enough (256 bins, 16 replicas: no slower
    // than noise), so those go without.
    const bool leaders = !LDS || a.log2_r < 3;
    const Vec16A* body = reinterpret_cast<const Vec16A*>(p + head);
    const int64_t steps = (nvec + kInfoStepVecs - 1) / kInfoStepVecs;
    int since = 0;
    for (int64_t s = blockIdx.x; s < steps; s += gridDim.x) {
        const int64_t v0 = s * kInfoStepVecs + threadIdx.x;
        Vec16A q[kInfoUnroll];
#pragma unroll
        for (int u = 0; u < kInfoUnroll; ++u) {
            const int64_t v = v0 + (int64_t)u * kInfoThreads;
            if (v < nvec) q[u] = body[v];
        }
#pragma unroll
        for (int u = 0; u < kInfoUnroll; ++u) {
            const int64_t v = v0 + (int64_t)u * kInfoThreads;
            if (v < nvec) {
                T e[PER];
                __builtin_memcpy(e, &q[u], 16);
                uint32_t b[PER];
                bool same = true;
#pragma unroll
                for (int i = 0; i < PER; ++i) {
                    b[i] = bin(e[i]);
                    same = same && b[i] == b[0];
                }
                // one bin for every element of the active lanes' vectors: one add of the count
                const uint32_t first = __builtin_amdgcn_readfirstlane(b[0]);
                if (__builtin_amdgcn_ballot_w64(!(same && b[0] == first)) == 0) {
                    const uint64_t active = __builtin_amdgcn_ballot_w64(true);
                    add_group(first, (uint32_t)__builtin_popcountll(active) * PER,
                              lane == __builtin_ctzll(active));
                } else if (!leaders) {
#pragma unroll
                    for (int i = 0; i < PER; ++i) add(b[i], 1u);
                } else {
                    // per element: the lanes that share the first active lane's bin (most of
                    // them over a background) add their count once; two rounds, then 1 each
#pragma unroll
                    for (int i = 0; i < PER; ++i) {
                        const uint32_t f = __builtin_amdgcn_readfirstlane(b[i]);
                        const uint64_t eq = __builtin_amdgcn_ballot_w64(b[i] == f);
                        add_group(f, (uint32_t)__builtin_popcountll(eq),
                                  lane == __builtin_ctzll(eq));
                        if (b[i] != f) {  // once more among the lanes that are left
                            const uint32_t g = __builtin_amdgcn_readfirstlane(b[i]);
                            const uint64_t eq2 = __builtin_amdgcn_ballot_w64(b[i] == g);
                            if (b[i] != g) add(b[i], 1u);
                            else if (lane == __builtin_ctzll(eq2))
                                add(g, (uint32_t)__builtin_popcountll(eq2));
                        }
                    }
                }
            }
        }
        if (++since == kInfoFlushSteps) {  // the same trip count in every lane of the workgroup
            flush();
            since = 0;
        }
    }
    if (blockIdx.x == 0) {  // head and tail: fewer than one vector each
        const int64_t t0 = head + nvec * PER;
        if ((int)threadIdx.x < head) add(bin(p[threadIdx.x]), 1u);
        if (t0 + threadIdx.x < n) add(bin(p[t0 + threadIdx.x]), 1u);
    }
    if constexpr (!LDS) {
        if (lane == 0 && pend_count) add(pend_bin, pend_count);
    }
    flush();
}

template <typename T>
hipError_t launch_range_t(const void* in, int64_t n, void* state, hipStream_t s) {
    int head;
    int64_t nvec;
    static const int resident = resident_blocks(range_kernel<T>);  // asked once
    const unsigned grid = split_run(resident, in, n, (int)sizeof(T), &head, &nvec);
    hipLaunchKernelGGL((range_kernel<T>), dim3(grid), dim3(kInfoThreads), 0, s,
                       static_cast<const T*>(in), n, head, nvec,
                       static_cast<unsigned long long*>(state));
    return hipGetLastError();
}

template <typename T, bool LDS>
hipError_t launch_hist_t(const void* in, int64_t n, const HistArgs& a, uint64_t* hist,
                         hipStream_t s) {
    int head;
    int64_t nvec;
    static const int resident = resident_blocks(hist_kernel<T, LDS>);  // asked once
    const unsigned grid = split_run(resident, in, n, (int)sizeof(T), &head, &nvec);
    hipLaunchKernelGGL((hist_kernel<T, LDS>), dim3(grid), dim3(kInfoThreads), 0, s,
                       static_cast<const T*>(in), n, head, nvec, a,
                       reinterpret_cast<unsigned long long*>(hist));
    return hipGetLastError();
}

}  // namespace

int info_max_blocks() {
    // about 8 workgroups of 256 threads per CU, as pointwise_max_blocks(); ZT_INFO_MAX_BLOCKS
    // lowers it (tests reach the grid-stride loop's second trip with a small array)
    if (const char* e = std::getenv("ZT_INFO_MAX_BLOCKS")) {
        const long v = std::atol(e);
        if (v >= 1 && v <= 65535) return (int)v;
    }
    return 2048;
}

hipError_t launch_range_init(void* state, hipStream_t s) {
    hipLaunchKernelGGL(range_init_kernel, dim3(1), dim3(1), 0, s,
                       static_cast<unsigned long long*>(state));
    return hipGetLastError();
}

hipError_t launch_range_accumulate(const void* in, int dtype, int64_t n, void* state,
                                   hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (dtype == kBool) return hipErrorInvalidValue;
    ZT_DISPATCH_DTYPE(dtype, T, return launch_range_t<T>(in, n, state, s))
    return hipErrorInvalidValue;
}

void range_decode(int dtype, uint64_t key, uint64_t* bits) {
    switch (dtype) {
    case kI8: *bits = (key ^ 0x80u) & 0xFFu; break;
    case kI16: *bits = (key ^ 0x8000u) & 0xFFFFu; break;
    case kI32: *bits = (key ^ 0x80000000u) & 0xFFFFFFFFu; break;
    case kI64: *bits = key ^ 0x8000000000000000ull; break;
    case kBF16: case kF16: *bits = ((key & 0x8000u) ? (key & 0x7FFFu) : ~key) & 0xFFFFu; break;
    case kF32: *bits = ((key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key) & 0xFFFFFFFFu; break;
    case kF64: *bits = (key >> 63) ? (key & 0x7FFFFFFFFFFFFFFFull) : ~key; break;
    default: *bits = key; break;
    }
}

hipError_t launch_histogram_accumulate(const void* in, int dtype, int64_t n, int64_t n_bins,
                                       double mn, double mx, uint64_t* hist, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (dtype == kBool || n_bins < 1 || n_bins > kInfoMaxBins) return hipErrorInvalidValue;
    HistArgs a;
    a.mn = mn;
    a.range = mx - mn;
    a.nb = (double)n_bins;
    a.last = (uint32_t)(n_bins - 1);
    a.n_bins = n_bins;
    a.log2_r = 0;
    if (n_bins <= kInfoLdsBins) {
        // replicas: the largest power of two with n_bins * R <= kInfoLdsBins, at most one per lane
        while (a.log2_r < 6 && (n_bins << (a.log2_r + 1)) <= kInfoLdsBins) ++a.log2_r;
        ZT_DISPATCH_DTYPE(dtype, T, return (launch_hist_t<T, true>(in, n, a, hist, s)))
    } else {
        ZT_DISPATCH_DTYPE(dtype, T, return (launch_hist_t<T, false>(in, n, a, hist, s)))
    }
    return hipErrorInvalidValue;
}

}  // namespace zt
