// distance.hip — the exact Euclidean distance transform (an extension: the reference has no such
// filter) for gfx950.
//
// The working state is g, one W per element (W = uint32_t, or uint64_t when the bound on the
// squared distance needs it): the squared distance to the nearest background element along the
// axes handled so far, all ones ("+inf": no background seen yet) otherwise.
//
//   edt_row_kernel    innermost axis. A wave owns a row and walks it in segments of 64 elements:
//                     a 64-bit word of the segment's background flags (a ballot, or assembled from
//                     16-byte loads), the nearest background to the left and right inside the
//                     segment from clz / ctz of the masked word, the nearest one in an earlier
//                     segment carried along; a backward sweep over g (whose zeros are the
//                     background) brings in the nearest one of a later segment.
//                     g = spacing_x^2 * dx^2 or +inf.
//   edt_axis_kernel   every further axis of extent > 1: f(i) = min_j g(j) + w * (i - j)^2 along
//                     every line of the axis, one lane per line, neighbouring lanes on
//                     neighbouring innermost positions, by the integer lower-envelope scan of
//                     Meijster, Roerdink and Hesselink. It reads one work array and writes the
//                     other, so g at an apex is still there after the line's results were written;
//                     the stack of a lane (apex position and breakpoint, one 8-byte slot) lives in
//                     device scratch laid out like the array (slot q of a line at the index of
//                     its element q).
//   edt_write_kernel  out = sqrt(g as f64) as TOut, or g itself (saturated) with `squared`.
//
// Termination: every loop is bounded by the line length. The forward scan of a line of n elements
// makes at most n pushes, so at most n pops in total, and the backward scan n steps. No kernel
// waits for another workgroup, uses an atomic or depends on the order workgroups run in; the
// dependency between the axes is the order of the launches on one stream.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <cstdlib>
#include <limits>
#include <type_traits>

#include "zt_device.hpp"
#include "zt_gpu.hpp"
#include "zt_edt_host.hpp"
#include "zt_kernels.hpp"

namespace zt {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
// Grids are capped at 2^22 threads, several times what the device holds at once; the kernels loop
// over the rest (a test reaches the loops with a few million rows, lines and output groups).
constexpr unsigned kMaxBlocks = 1u << 14;


// ---- innermost axis ----------------------------------------------------------------------------

// One segment of a row: `word` holds the background flags of elements x0 .. x0 + 63 (no bit set at
// or beyond the row's end), `carry` the nearest background x before x0 or -1. The sentinel stays
// where the row has had no background so far; the backward sweep looks at what comes later.
template <typename W>
__device__ inline void row_segment(W* __restrict__ grow, int x0, int lane, int X, uint64_t word,
                                   int& carry, W w) {
    const int x = x0 + lane;
    const uint64_t below = word & ((2ull << lane) - 1);   // flags at lanes <= this one
    const uint64_t above = word & ~((1ull << lane) - 1);  // flags at lanes >= this one
    const int xl = below ? x0 + 63 - __clzll((long long)below) : carry;
    uint32_t d = 0xFFFFFFFFu;
    if (xl >= 0) d = (uint32_t)(x - xl);
    if (above) {
        const uint32_t dr = (uint32_t)(x0 + __builtin_ctzll(above) - x);
        d = dr < d ? dr : d;
    }
    if (x < X) grow[x] = d == 0xFFFFFFFFu ? ~(W)0 : (W)(w * ((W)d * (W)d));
    if (word) carry = x0 + 63 - __clzll((long long)word);
}

template <int ESZ, typename W>
__global__ __launch_bounds__(kThreads) void edt_row_kernel(const uint8_t* __restrict__ in,
                                                           W* __restrict__ g, int64_t rows, int X,
                                                           uint64_t fgmask, W w, int vec_ok) {
    using U = typename UIntOf<ESZ>::type;
    constexpr int kPer = 16 / ESZ;        // elements of a 16-byte piece = segments of a group
    constexpr int kLanesPerSeg = 64 / kPer;
    const int lane = threadIdx.x & 63;
    const U m = (U)fgmask;
    const int nseg = (X + 63) / 64;
    for (int64_t row = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); row < rows;
         row += (int64_t)gridDim.x * kWaves) {
        const U* src = reinterpret_cast<const U*>(in) + row * X;
        W* grow = g + row * X;
        int carry = -1, seg = 0;
        if (vec_ok) {
            // a group: 64 lanes x 16 bytes = kPer segments; lane l holds the elements
            // kPer * l .. kPer * l + kPer - 1 of the group, their flags in the low bits of `bits`
            for (; (int64_t)(seg + kPer) * 64 <= X; seg += kPer) {
                const uint4 v = *reinterpret_cast<const uint4*>(
                    reinterpret_cast<const uint8_t*>(src + (int64_t)seg * 64) + lane * 16);
                const uint32_t wv[4] = {v.x, v.y, v.z, v.w};
                uint32_t bits = 0;
#pragma unroll
                for (int j = 0; j < kPer; ++j) {
                    U e;
                    if constexpr (ESZ == 8) e = (U)wv[2 * j] | ((U)wv[2 * j + 1] << 32);
                    else e = (U)(wv[j * ESZ / 4] >> (8 * ((j * ESZ) % 4)));
                    bits |= (uint32_t)((e & m) == 0) << j;
                }
#pragma unroll
                for (int k = 0; k < kPer; ++k) {
                    uint64_t word = 0;
#pragma unroll
                    for (int j = 0; j < kLanesPerSeg; ++j)
                        word |= (uint64_t)(uint32_t)__builtin_amdgcn_readlane(
                                    (int)bits, k * kLanesPerSeg + j)
                                << (j * kPer);
                    row_segment<W>(grow, (seg + k) * 64, lane, X, word, carry, w);
                }
            }
        }
        for (; seg < nseg; ++seg) {
            const int x = seg * 64 + lane;
            const bool bg = x < X && (src[x] & m) == 0;
            row_segment<W>(grow, seg * 64, lane, X, __ballot(bg), carry, w);
        }
        if (nseg == 1) continue;
        // backward: the zeros of g are the background. Only the elements behind the last
        // background of their segment can have a nearer one in a later segment.
        int next = -1;
        for (seg = nseg - 1; seg >= 0; --seg) {
            const int x = seg * 64 + lane;
            const W gv = x < X ? grow[x] : ~(W)0;
            const uint64_t word = __ballot(gv == 0);
            if (next >= 0 && x < X) {
                const int hi = word ? 63 - __clzll((long long)word) : -1;
                if (lane > hi) {
                    const uint32_t d = (uint32_t)(next - x);
                    const W g2 = (W)(w * ((W)d * (W)d));
                    if (g2 < gv) grow[x] = g2;
                }
            }
            if (word) next = seg * 64 + __builtin_ctzll(word);
        }
    }
}

// ---- further axes ------------------------------------------------------------------------------

// The parabola of apex i with value gi, at x: gi + w * (x - i)^2. Never called with the sentinel.
template <typename W>
__device__ inline W parabola(W gi, W w, int x, int i) {
    const uint32_t d = (uint32_t)(x > i ? x - i : i - x);
    return gi + w * ((W)d * (W)d);
}

// The largest x at which apex i (value gi) is not above apex u > i (value gu):
// floor((w * (u^2 - i^2) + gu - gi) / (2 * w * (u - i))). The caller has just seen apex i not above
// apex u at a breakpoint >= 0, so the numerator is not negative. With W = uint32_t the numerator is
// below 2^33 and w * (u - i) below 2^32, and floor(a / (2 d)) = floor(floor(a / 2) / d): one 32-bit
// division. With W = uint64_t it is a 64-bit division, a long software routine on this GPU; both
// run once per push, never in the pop loop.
template <typename W>
__device__ inline uint64_t separator(W gi, W gu, W w, int i, int u) {
    const uint64_t half_den = (uint64_t)w * (uint32_t)(u - i);
    const uint64_t num = half_den * (uint32_t)(u + i) + (uint64_t)gu - (uint64_t)gi;
    if constexpr (sizeof(W) == 4) return (uint32_t)(num >> 1) / (uint32_t)half_den;
    else return num / (2 * half_den);
}

template <typename W>
__global__ __launch_bounds__(kThreads) void edt_axis_kernel(const W* __restrict__ gin,
                                                            W* __restrict__ gout,
                                                            uint2* __restrict__ stack,
                                                            int64_t lines, int64_t inner, int na,
                                                            W w) {
    constexpr W kInf = ~(W)0;
    for (int64_t line = (int64_t)blockIdx.x * kThreads + threadIdx.x; line < lines;
         line += (int64_t)gridDim.x * kThreads) {
        const int64_t base = (line / inner) * na * inner + line % inner;
        const W* gi = gin + base;
        W* go = gout + base;
        uint2* st = stack + base;  // slot q: (apex position, breakpoint), one 8-byte access
        // the top of the stack in registers: apex cs with value cg, lowest from breakpoint ct on
        int q = -1, cs = 0, ct = 0;
        W cg = 0;
        W ahead = gi[0];  // the next site's value, loaded one step early
        for (int u = 0; u < na; ++u) {
            const W gu = ahead;
            if (u + 1 < na) ahead = gi[(int64_t)(u + 1) * inner];
            if (gu == kInf) continue;  // a sentinel site is never pushed
            while (q >= 0 && parabola<W>(cg, w, ct, cs) > parabola<W>(gu, w, ct, u)) {
                if (--q >= 0) {
                    const uint2 e = st[(int64_t)q * inner];
                    cs = (int)e.x;
                    ct = (int)e.y;
                    cg = gi[(int64_t)cs * inner];
                }
            }
            if (q < 0) {
                q = 0;
                ct = 0;
            } else {
                const uint64_t from = separator<W>(cg, gu, w, cs, u) + 1;
                if (from >= (uint64_t)na) continue;  // u is lowest nowhere on the line
                ++q;
                ct = (int)from;
            }
            cs = u;
            cg = gu;
            st[(int64_t)q * inner] = make_uint2((uint32_t)cs, (uint32_t)ct);
        }
        if (q < 0) {  // a line of sentinels stays sentinels
            for (int u = 0; u < na; ++u) go[(int64_t)u * inner] = kInf;
            continue;
        }
        for (int u = na - 1; u >= 0; --u) {
            go[(int64_t)u * inner] = parabola<W>(cg, w, u, cs);
            if (u == ct && --q >= 0) {
                const uint2 e = st[(int64_t)q * inner];
                cs = (int)e.x;
                ct = (int)e.y;
                cg = gi[(int64_t)cs * inner];
            }
        }
    }
}

// ---- write -------------------------------------------------------------------------------------

template <typename W, typename TOut>
__device__ inline TOut edt_value(W gv, int squared) {
    if (gv == ~(W)0) return as_cast<double, TOut>(INFINITY);  // the type's maximum for integers
    if (!squared) return as_cast<double, TOut>(__builtin_sqrt((double)gv));
    if constexpr (std::is_integral_v<TOut>) {
        constexpr uint64_t most = (uint64_t)std::numeric_limits<TOut>::max();
        return (uint64_t)gv > most ? (TOut)most : (TOut)gv;
    } else {
        return as_cast<double, TOut>((double)gv);
    }
}

template <typename W, typename TOut>
__global__ __launch_bounds__(kThreads) void edt_write_kernel(const W* __restrict__ g,
                                                             TOut* __restrict__ out, int64_t n,
                                                             int squared, int vec_ok) {
    constexpr int kPer = 16 / (int)sizeof(TOut);
    using U = typename UIntOf<sizeof(TOut)>::type;
    const int64_t groups = (n + kPer - 1) / kPer;
    for (int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x; t < groups;
         t += (int64_t)gridDim.x * kThreads) {
        const int64_t i0 = t * kPer;
        if (vec_ok && i0 + kPer <= n) {
            uint32_t p[4] = {0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < kPer; ++j) {
                const U b = __builtin_bit_cast(U, edt_value<W, TOut>(g[i0 + j], squared));
                if constexpr (sizeof(TOut) == 8) {
                    p[2 * j] = (uint32_t)b;
                    p[2 * j + 1] = (uint32_t)((uint64_t)b >> 32);
                } else {
                    p[j * (int)sizeof(TOut) / 4] |= (uint32_t)b
                                                    << (8 * ((j * (int)sizeof(TOut)) % 4));
                }
            }
            *reinterpret_cast<uint4*>(out + i0) = make_uint4(p[0], p[1], p[2], p[3]);
        } else {
            for (int j = 0; j < kPer && i0 + j < n; ++j)
                out[i0 + j] = edt_value<W, TOut>(g[i0 + j], squared);
        }
    }
}

// ---- host ----------------------------------------------------------------------------------------

unsigned grid_for(int64_t items, int per_block) {
    const int64_t b = (items + per_block - 1) / per_block;
    return (unsigned)(b < 1 ? 1 : b > (int64_t)kMaxBlocks ? (int64_t)kMaxBlocks : b);
}

template <typename W>
hipError_t edt_run(const void* in, int dtype_in, const int64_t* shape, int ndim,
                   const uint64_t* weight, void* scratch, void* out, int dtype_out, int squared,
                   hipStream_t s) {
    int64_t n = 1;
    for (int a = 0; a < ndim; ++a) n *= shape[a];
    W* cur = static_cast<W*>(scratch);
    W* other = cur + n;
    uint2* stack = reinterpret_cast<uint2*>(other + n);  // 8-byte aligned: 2 * n * sizeof(W) in

    const int X = (int)shape[ndim - 1];
    const int64_t rows = n / X;
    const int esz = (int)dtype_size(dtype_in);
    const int vec_ok = ((uintptr_t)in % 16 == 0) && ((uint64_t)X * esz) % 16 == 0;
    const uint64_t mask = fg_mask(dtype_in);
    const uint8_t* src = static_cast<const uint8_t*>(in);
    const W wx = (W)weight[ndim - 1];
    const unsigned rg = grid_for(rows, kWaves);
    switch (esz) {
    case 1: edt_row_kernel<1, W><<<rg, kThreads, 0, s>>>(src, cur, rows, X, mask, wx, vec_ok); break;
    case 2: edt_row_kernel<2, W><<<rg, kThreads, 0, s>>>(src, cur, rows, X, mask, wx, vec_ok); break;
    case 4: edt_row_kernel<4, W><<<rg, kThreads, 0, s>>>(src, cur, rows, X, mask, wx, vec_ok); break;
    case 8: edt_row_kernel<8, W><<<rg, kThreads, 0, s>>>(src, cur, rows, X, mask, wx, vec_ok); break;
    default: return hipErrorInvalidValue;
    }
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;

    int64_t inner = X;
    for (int a = ndim - 2; a >= 0; inner *= shape[a], --a) {
        if (shape[a] <= 1) continue;
        const int64_t lines = n / shape[a];
        edt_axis_kernel<W><<<grid_for(lines, kThreads), kThreads, 0, s>>>(
            cur, other, stack, lines, inner, (int)shape[a], (W)weight[a]);
        W* t = cur;
        cur = other;
        other = t;
    }
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;

    const int out_vec = (uintptr_t)out % 16 == 0;
    ZT_DISPATCH_DTYPE(dtype_out, TOut, {
        constexpr int kPer = 16 / (int)sizeof(TOut);
        edt_write_kernel<W, TOut><<<grid_for((n + kPer - 1) / kPer, kThreads), kThreads, 0, s>>>(
            cur, static_cast<TOut*>(out), n, squared, out_vec);
    });
    return hipGetLastError();
}

}  // namespace

bool edt_work64(bool needed) {
    // ZT_EDT_WORK64=1 forces the 64-bit instantiation (tests reach it with a small array)
    if (const char* e = std::getenv("ZT_EDT_WORK64"))
        if (e[0] == '1' && e[1] == 0) return true;
    return needed;
}

hipError_t launch_edt(const void* in, int dtype_in, const int64_t* shape, int ndim,
                      const uint64_t* weight, bool work64, void* scratch, void* out, int dtype_out,
                      int squared, hipStream_t s) {
    return work64 ? edt_run<uint64_t>(in, dtype_in, shape, ndim, weight, scratch, out, dtype_out,
                                      squared, s)
                  : edt_run<uint32_t>(in, dtype_in, shape, ndim, weight, scratch, out, dtype_out,
                                      squared, s);
}

}  // namespace zt
