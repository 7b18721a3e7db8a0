// sat.hip — summed-area table (summed_area_table.rs:47-106, :144-253): one inclusive running sum
// per axis, last axis first, in the output type. For the axis being scanned the array is
// outer x n x inner; a lane is one (outer, inner) position and is always folded left to right by
// one thread, `element += acc` from the seed on (:94-97), so float results carry the reference's
// rounding order. Parallelism comes from the lanes alone.
//   inner == 1 (the x scan): sat_x_kernel. A workgroup owns kSatRows rows and marches along x in
//     tiles of W columns: coalesced load (TIn -> TOut on the way in) into LDS, one thread per row
//     folds its W elements from the carry it keeps in a register, coalesced store; the next
//     tile's loads are issued before the fold (DESIGN.md 3.6 has the measurements).
//   inner  > 1: sat_strided_kernel, in place. Consecutive threads take consecutive inner, so
//     every access is coalesced; each thread walks n with stride inner.
// Both take an optional seed per lane (in place of zero) and leave the lane's last value.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "zt_device.hpp"
#include "zt_kernels.hpp"

namespace zt {

namespace {

// `element += acc` in TOut. Integers wrap (Rust release builds; debug builds panic on overflow):
// the add runs on the unsigned type of the same size. f16 / bf16: half's `+` is an f32 add
// rounded back with from_f32, once per add.
template <typename T>
__device__ inline T sat_add(T e, T acc) {
    if constexpr (kIsHalf<T>) {
        return from_f32<T>(Elem<T>::to_f32(e) + Elem<T>::to_f32(acc));
    } else if constexpr (std::is_integral_v<T>) {
        using U = std::make_unsigned_t<T>;
        return (T)(U)((U)e + (U)acc);
    } else {
        return e + acc;
    }
}

template <typename T>
__device__ inline T sat_zero() {
    if constexpr (kIsHalf<T>) return T{0};
    else return (T)0;
}

// LDS tile of the x scan: kSatRows rows of W elements, W * sizeof(TOut) = 128 B of a row per
// tile (64 B and 32 B for the 2- and 1-byte types). Rows are padded to an odd number of dwords
// (two dwords more for 8-byte elements), so the row-per-thread walk of the fold touches 32
// distinct banks per 32 lanes with ds_read_b32 / ds_write_b32 (pitch 33 dwords: bank 33 t mod
// 32 = t), and all 64 banks with ds_read_b64 (pitch 34 dwords: 34 t mod 64 runs through the even
// banks once for t = 0..31, each lane taking that bank and the next; ds_write_b64 groups 16
// lanes on 32 banks: 2 t mod 32).
template <typename TO>
struct SatTile {
    static constexpr int W = sizeof(TO) == 8 ? kSatTileW8 : kSatTileW;
    static constexpr int PAD = sizeof(TO) >= 4 ? 1 : 4 / (int)sizeof(TO);
    static constexpr int PITCH = W + PAD;
};

template <typename TI, typename TO>
__global__ __launch_bounds__(kSatThreads) void sat_x_kernel(const TI* in, TO* out, int64_t rows,
                                                            int64_t n, const TO* seed, TO* last) {
    constexpr int W = SatTile<TO>::W, PITCH = SatTile<TO>::PITCH;
    constexpr int RS = kSatThreads / W;  // rows covered by one load / store step
    __shared__ TO tile[kSatRows * PITCH];
    const int tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * kSatRows;
    const int nrows = (int)(rows - row0 < kSatRows ? rows - row0 : kSatRows);
    const int col = tid % W, rsub = tid / W;
    TO acc = sat_zero<TO>();
    if (seed && tid < nrows) acc = seed[row0 + tid];
    // `in` may be `out` (a later pass with inner == 1): a tile is loaded whole before it is
    // stored, element by the thread that loaded it, and tiles do not overlap.
    // The next tile's global loads are issued into registers before this tile is folded and
    // stored, so they are in flight meanwhile.
    constexpr int NR = kSatRows / RS;  // elements per thread and tile
    TI pre[NR];
    auto prefetch = [&](int64_t x0) {
        const int w = (int)(n - x0 < W ? n - x0 : W);
        if (col < w) {
#pragma unroll
            for (int k = 0; k < NR; ++k) {
                const int r = rsub + k * RS;
                if (r < nrows) pre[k] = in[(row0 + r) * n + x0 + col];
            }
        }
    };
    if (n > 0) prefetch(0);
    for (int64_t x0 = 0; x0 < n; x0 += W) {
        const int w = (int)(n - x0 < W ? n - x0 : W);
        if (col < w) {
#pragma unroll
            for (int k = 0; k < NR; ++k) {
                const int r = rsub + k * RS;
                if (r < nrows) tile[r * PITCH + col] = as_cast<TI, TO>(pre[k]);
            }
        }
        __syncthreads();
        if (x0 + W < n) prefetch(x0 + W);
        if (tid < nrows) {
            TO* t = tile + tid * PITCH;
            if (w == W) {
#pragma unroll
                for (int c = 0; c < W; ++c) {
                    acc = sat_add<TO>(t[c], acc);
                    t[c] = acc;
                }
            } else {
                for (int c = 0; c < w; ++c) {
                    acc = sat_add<TO>(t[c], acc);
                    t[c] = acc;
                }
            }
        }
        __syncthreads();
        // the next tile's LDS writes overwrite only what this thread reads here: no third
        // barrier
        if (col < w) {
#pragma unroll
            for (int k = 0; k < NR; ++k) {
                const int r = rsub + k * RS;
                if (r < nrows) out[(row0 + r) * n + x0 + col] = tile[r * PITCH + col];
            }
        }
    }
    if (last && tid < nrows) last[row0 + tid] = acc;
}

// One thread per lane; U elements are loaded before the dependent adds so U loads are in flight.
template <typename TO>
__global__ __launch_bounds__(kSatThreads) void sat_strided_kernel(TO* data, int64_t outer,
                                                                  int64_t n, int64_t inner,
                                                                  const TO* seed, TO* last) {
    constexpr int U = 8;
    const int64_t lane = (int64_t)blockIdx.x * kSatThreads + threadIdx.x;
    if (lane >= outer * inner) return;
    const int64_t o = lane / inner, i = lane - o * inner;
    TO* p = data + o * n * inner + i;
    TO acc = seed ? seed[lane] : sat_zero<TO>();
    int64_t k = 0;
    for (; k + U <= n; k += U) {
        TO v[U];
#pragma unroll
        for (int j = 0; j < U; ++j) v[j] = p[(k + j) * inner];
#pragma unroll
        for (int j = 0; j < U; ++j) {
            acc = sat_add<TO>(v[j], acc);
            p[(k + j) * inner] = acc;
        }
    }
    for (; k < n; ++k) {
        acc = sat_add<TO>(p[k * inner], acc);
        p[k * inner] = acc;
    }
    if (last) last[lane] = acc;  // `last` may be `seed`: read above by this thread only
}

// The in-place passes depend on TOut's size and arithmetic only: integers of one size share the
// unsigned instantiation (wrapping add), which leaves 8.
#define ZT_SAT_DISPATCH_ARITH(CODE, T, ...)                                                     \
    switch (CODE) {                                                                             \
    case kBool: case kU8: case kI8: { using T = uint8_t; __VA_ARGS__; } break;                  \
    case kU16: case kI16: { using T = uint16_t; __VA_ARGS__; } break;                           \
    case kU32: case kI32: { using T = uint32_t; __VA_ARGS__; } break;                           \
    case kU64: case kI64: { using T = uint64_t; __VA_ARGS__; } break;                           \
    case kBF16: { using T = bf16_t; __VA_ARGS__; } break;                                       \
    case kF16: { using T = f16_t; __VA_ARGS__; } break;                                         \
    case kF32: { using T = float; __VA_ARGS__; } break;                                         \
    case kF64: { using T = double; __VA_ARGS__; } break;                                        \
    default: break;                                                                             \
    }

}  // namespace

hipError_t launch_sat_pass(const void* in, int dtype_in, void* out, int dtype_out, int64_t outer,
                           int64_t n, int64_t inner, const void* seed, void* last, hipStream_t s) {
    if (outer <= 0 || n <= 0 || inner <= 0) return hipSuccess;
    const bool in_place = in == out;
    if (in_place && dtype_in != dtype_out) return hipErrorInvalidValue;
    if (inner > 1 && !in_place) return hipErrorInvalidValue;
    const int64_t lanes = outer * inner;
    const int64_t per = inner == 1 ? kSatRows : kSatThreads;
    const int64_t blocks = (lanes + per - 1) / per;
    if (blocks > INT32_MAX) return hipErrorInvalidValue;
    hipError_t err = hipErrorInvalidValue;
    if (in_place) {
        ZT_SAT_DISPATCH_ARITH(dtype_out, TO,
            if (inner == 1)
                hipLaunchKernelGGL((sat_x_kernel<TO, TO>), dim3((unsigned)blocks),
                                   dim3(kSatThreads), 0, s, static_cast<const TO*>(in),
                                   static_cast<TO*>(out), outer, n, static_cast<const TO*>(seed),
                                   static_cast<TO*>(last));
            else
                hipLaunchKernelGGL((sat_strided_kernel<TO>), dim3((unsigned)blocks),
                                   dim3(kSatThreads), 0, s, static_cast<TO*>(out), outer, n,
                                   inner, static_cast<const TO*>(seed), static_cast<TO*>(last));
            err = hipGetLastError())
        return err;
    }
    ZT_DISPATCH_DTYPE(dtype_in, TI,
        ZT_DISPATCH_DTYPE(dtype_out, TO,
            hipLaunchKernelGGL((sat_x_kernel<TI, TO>), dim3((unsigned)blocks), dim3(kSatThreads),
                               0, s, static_cast<const TI*>(in), static_cast<TO*>(out), outer, n,
                               static_cast<const TO*>(seed), static_cast<TO*>(last));
            err = hipGetLastError()))
    return err;
}

}  // namespace zt
