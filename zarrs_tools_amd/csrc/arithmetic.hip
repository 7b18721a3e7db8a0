// arithmetic.hip — the two-array arithmetic filter (an extension: the reference has no such
// filter): out[i] = (first[i] as f64  op  second[i] as f64) as TOut over n contiguous elements,
// op one of add, subtract, multiply, divide, minimum, maximum, absolute_difference.
//
// `as` is Rust's, written once in as_cast (zt_device.hpp): every operand is widened to f64 at the
// load (exact but for 64-bit integers above 2^53, which round to nearest even), the operator is
// one IEEE f64 operation (no contraction, denormals kept), and the result goes through the final
// cast of rescale (pointwise.hip): float -> integer saturates, NaN -> 0, f64 -> half in one
// rounding, bool written as u8. minimum / maximum are a compare and a select, `y < x ? y : x` and
// `y > x ? y : x`: a NaN on either side, or +-0 against -+0, returns x.
//
// The kernel follows pointwise.hip. It is templated on the three element sizes, not on type
// triples: the data types and the operator are kernel arguments, wave-uniform, their branches
// uniform and outside the element loops. Each lane carries 16 elements per step, as U vectors of
// V = 16 / (smallest of the three sizes) elements, 256 vectors apart so that a wave's accesses are
// contiguous. The stream with the smallest element (the output on a tie, then the first input)
// is accessed as one aligned 16-byte vector per lane, the other streams as V * size / 16 16-byte
// vectors at element alignment (gfx950 global accesses in unaligned mode). The elements before
// the first aligned vector and after the last whole one (fewer than V each) go element by element
// in workgroup 0. Every address comes from an index in [0, n). The first operand's 16 elements are
// widened to f64 together; the second operand's are widened inside the operator's loop, one at a
// time (holding both as f64 cost 12-26 more VGPRs and 7-22 % more time per byte).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdlib>
#include <type_traits>

#include "zt_device.hpp"
#include "zt_info.hpp"
#include "zt_kernels.hpp"

namespace zt {

namespace {

constexpr int kArElems = kArStepElems / kArThreads;  // elements a lane carries per step
static_assert(kArThreads == kInfoThreads, "resident_blocks (zt_info.hpp) asks for that many");

template <typename T> struct Tag { using type = T; };

// f(Tag<T>) for the element type T of `dt`, one of the types of SZ bytes (bool as u8)
template <int SZ, typename F>
__device__ __forceinline__ void by_type(int dt, F&& f) {
    if constexpr (SZ == 1) {
        if (dt == kI8) f(Tag<int8_t>{});
        else f(Tag<uint8_t>{});
    } else if constexpr (SZ == 2) {
        if (dt == kI16) f(Tag<int16_t>{});
        else if (dt == kF16) f(Tag<f16_t>{});
        else if (dt == kBF16) f(Tag<bf16_t>{});
        else f(Tag<uint16_t>{});
    } else if constexpr (SZ == 4) {
        if (dt == kI32) f(Tag<int32_t>{});
        else if (dt == kF32) f(Tag<float>{});
        else f(Tag<uint32_t>{});
    } else {
        if (dt == kI64) f(Tag<int64_t>{});
        else if (dt == kF64) f(Tag<double>{});
        else f(Tag<uint64_t>{});
    }
}

// storage bits (zero-extended) -> `v as f64`
template <typename T>
__device__ __forceinline__ double bits_to_f64(uint64_t b) {
    if constexpr (std::is_same_v<T, bf16_t>) return (double)bf16_bits_to_f32((uint16_t)b);
    else if constexpr (std::is_same_v<T, f16_t>) return (double)f16_bits_to_f32((uint16_t)b);
    else if constexpr (std::is_same_v<T, float>) return (double)u2f((uint32_t)b);
    else if constexpr (std::is_same_v<T, double>) return __builtin_bit_cast(double, b);
    else return (double)(T)b;  // i64 / u64: round to nearest even
}

// `r as T` -> storage bits (zero-extended)
template <typename T>
__device__ __forceinline__ uint64_t f64_to_bits(double r) {
    const T t = as_cast<double, T>(r);
    if constexpr (kIsHalf<T>) return t.bits;
    else if constexpr (std::is_same_v<T, float>) return f2u(t);
    else if constexpr (std::is_same_v<T, double>) return d2u(t);
    else return (uint64_t)(std::make_unsigned_t<T>)t;
}

// N elements of SZ bytes, packed as in memory, in 32-bit words
template <int SZ, int N>
struct Words {
    uint32_t w[(N * SZ + 3) / 4];
};

template <int SZ, int N>
__device__ __forceinline__ uint64_t get_bits(const Words<SZ, N>& q, int e) {
    if constexpr (SZ == 1) return (q.w[e / 4] >> (8 * (e % 4))) & 0xFFu;
    else if constexpr (SZ == 2) return (q.w[e / 2] >> (16 * (e % 2))) & 0xFFFFu;
    else if constexpr (SZ == 4) return q.w[e];
    else return ((uint64_t)q.w[2 * e + 1] << 32) | q.w[2 * e];
}

template <int SZ, int N>
__device__ __forceinline__ void widen(const Words<SZ, N>& q, int dt, double (&x)[N]) {
    by_type<SZ>(dt, [&](auto tag) {
        using T = typename decltype(tag)::type;
#pragma unroll
        for (int e = 0; e < N; ++e) x[e] = bits_to_f64<T>(get_bits(q, e));
    });
}

template <int SZ, int N>
__device__ __forceinline__ void narrow(const double (&r)[N], int dt, Words<SZ, N>& q) {
#pragma unroll
    for (int i = 0; i < (N * SZ + 3) / 4; ++i) q.w[i] = 0;
    by_type<SZ>(dt, [&](auto tag) {
        using T = typename decltype(tag)::type;
#pragma unroll
        for (int e = 0; e < N; ++e) {
            const uint64_t b = f64_to_bits<T>(r[e]);
            if constexpr (SZ == 1) q.w[e / 4] |= (uint32_t)b << (8 * (e % 4));
            else if constexpr (SZ == 2) q.w[e / 2] |= (uint32_t)b << (16 * (e % 2));
            else if constexpr (SZ == 4) q.w[e] = (uint32_t)b;
            else { q.w[2 * e] = (uint32_t)b; q.w[2 * e + 1] = (uint32_t)(b >> 32); }
        }
    });
}

// x = x op (q as f64): one f64 operation per element. The second operand is widened where it is
// used, so that its 16 f64 values are never all live (32 VGPRs less than widening it first).
template <int SZ, int N>
__device__ __forceinline__ void apply_op(int op, double (&x)[N], const Words<SZ, N>& q, int dt) {
#pragma clang fp contract(off)
#define ZT_AR_LOOP(EXPR)                                                                         \
    by_type<SZ>(dt, [&](auto tag) {                                                              \
        using T = typename decltype(tag)::type;                                                  \
        _Pragma("unroll") for (int e = 0; e < N; ++e) {                                          \
            const double a = x[e], b = bits_to_f64<T>(get_bits(q, e));                           \
            x[e] = (EXPR);                                                                       \
        }                                                                                        \
    });
    switch (op) {
    case kArAdd: ZT_AR_LOOP(a + b) break;
    case kArSubtract: ZT_AR_LOOP(a - b) break;
    case kArMultiply: ZT_AR_LOOP(a * b) break;
    case kArDivide: ZT_AR_LOOP(a / b) break;
    case kArMinimum: ZT_AR_LOOP(b < a ? b : a) break;
    case kArMaximum: ZT_AR_LOOP(b > a ? b : a) break;
    default: ZT_AR_LOOP(__builtin_fabs(a - b)) break;  // kArAbsoluteDifference
    }
#undef ZT_AR_LOOP
}

// 16 bytes at alignment A (gfx950 global accesses take any alignment: unaligned access mode)
template <int A>
struct __attribute__((packed, aligned(A))) Vec16 {
    uint32_t w[4];
};

template <int SZ> struct Store;
template <> struct Store<1> { using type = uint8_t; };
template <> struct Store<2> { using type = uint16_t; };
template <> struct Store<4> { using type = uint32_t; };
template <> struct Store<8> { using type = uint64_t; };

// V elements of SZ bytes at p (16-byte vectors at alignment A) <-> the words from q.w[w0] on
template <int SZ, int A, int V, int N>
__device__ __forceinline__ void load_vec(const uint8_t* p, Words<SZ, N>& q, int w0) {
#pragma unroll
    for (int i = 0; i < V * SZ / 16; ++i) {
        const Vec16<A> t = *reinterpret_cast<const Vec16<A>*>(p + 16 * i);
#pragma unroll
        for (int k = 0; k < 4; ++k) q.w[w0 + 4 * i + k] = t.w[k];
    }
}

template <int SZ, int A, int V, int N>
__device__ __forceinline__ void store_vec(uint8_t* p, const Words<SZ, N>& q, int w0) {
#pragma unroll
    for (int i = 0; i < V * SZ / 16; ++i) {
        Vec16<A> t;
#pragma unroll
        for (int k = 0; k < 4; ++k) t.w[k] = q.w[w0 + 4 * i + k];
        *reinterpret_cast<Vec16<A>*>(p + 16 * i) = t;
    }
}

struct ArArgs {
    const uint8_t* a;
    const uint8_t* b;
    uint8_t* out;
    int64_t n, nvec;  // elements; whole vectors after the head
    int32_t head;     // elements before the first vector, < V
    int32_t op, dt_a, dt_b, dt_out;
};

// element i on its own (the head and the tail)
template <int SA, int SB, int SO>
__device__ __forceinline__ void one_element(const ArArgs& g, int64_t i) {
    using TA = typename Store<SA>::type;
    using TB = typename Store<SB>::type;
    using TO = typename Store<SO>::type;
    const uint64_t ba = reinterpret_cast<const TA*>(g.a)[i];
    const uint64_t bb = reinterpret_cast<const TB*>(g.b)[i];
    double x[1] = {0.0};
    by_type<SA>(g.dt_a, [&](auto tag) { x[0] = bits_to_f64<typename decltype(tag)::type>(ba); });
    Words<SB, 1> qb;
    qb.w[0] = (uint32_t)bb;
    if constexpr (SB == 8) qb.w[1] = (uint32_t)(bb >> 32);
    apply_op(g.op, x, qb, g.dt_b);
    uint64_t bo = 0;
    by_type<SO>(g.dt_out, [&](auto tag) { bo = f64_to_bits<typename decltype(tag)::type>(x[0]); });
    reinterpret_cast<TO*>(g.out)[i] = (TO)bo;
}

// A workgroup step is kArThreads * U vectors = kArStepElems elements; steps are grid-strided. In
// a step that lies whole inside the vectors (every step but the last) the U loads of a stream are
// issued together with no per-vector branch; the last step checks every vector and computes on
// zeros where a lane has none.
template <int SA, int SB, int SO>
__global__ __launch_bounds__(kArThreads) void arithmetic_kernel(const ArArgs g) {
    constexpr int SMIN = SA < SB ? (SA < SO ? SA : SO) : (SB < SO ? SB : SO);
    constexpr int V = 16 / SMIN, U = kArElems / V, E = kArElems;
    constexpr int kAligned = SO == SMIN ? 2 : (SA == SMIN ? 0 : 1);
    constexpr int AA = kAligned == 0 ? 16 : SA, AB = kAligned == 1 ? 16 : SB;
    constexpr int AO = kAligned == 2 ? 16 : SO;
    constexpr int64_t kStepVecs = (int64_t)kArThreads * U;
    const int64_t steps = (g.nvec + kStepVecs - 1) / kStepVecs;
    for (int64_t s = blockIdx.x; s < steps; s += gridDim.x) {
        const int64_t v0 = s * kStepVecs + threadIdx.x;
        const bool whole = (s + 1) * kStepVecs <= g.nvec;  // uniform over the workgroup
        const int64_t e0 = g.head + v0 * V;                // the lane's first element
        Words<SA, E> qa;
        Words<SB, E> qb;
        if (whole) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t e = e0 + (int64_t)u * kArThreads * V;
                load_vec<SA, AA, V>(g.a + e * SA, qa, u * V * SA / 4);
                load_vec<SB, AB, V>(g.b + e * SB, qb, u * V * SB / 4);
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4 * SA; ++i) qa.w[i] = 0;
#pragma unroll
            for (int i = 0; i < 4 * SB; ++i) qb.w[i] = 0;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (v0 + (int64_t)u * kArThreads < g.nvec) {
                    const int64_t e = e0 + (int64_t)u * kArThreads * V;
                    load_vec<SA, AA, V>(g.a + e * SA, qa, u * V * SA / 4);
                    load_vec<SB, AB, V>(g.b + e * SB, qb, u * V * SB / 4);
                }
            }
        }
        double x[E];
        widen(qa, g.dt_a, x);
        apply_op(g.op, x, qb, g.dt_b);
        Words<SO, E> qo;
        narrow(x, g.dt_out, qo);
        if (whole) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t e = e0 + (int64_t)u * kArThreads * V;
                store_vec<SO, AO, V>(g.out + e * SO, qo, u * V * SO / 4);
            }
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (v0 + (int64_t)u * kArThreads < g.nvec) {
                    const int64_t e = e0 + (int64_t)u * kArThreads * V;
                    store_vec<SO, AO, V>(g.out + e * SO, qo, u * V * SO / 4);
                }
            }
        }
    }
    if (blockIdx.x == 0) {  // head and tail: fewer than one vector each
        const int64_t t0 = g.head + g.nvec * V;
        if ((int)threadIdx.x < g.head) one_element<SA, SB, SO>(g, threadIdx.x);
        if (t0 + threadIdx.x < g.n) one_element<SA, SB, SO>(g, t0 + threadIdx.x);
    }
}

template <int SA, int SB, int SO>
hipError_t launch_one(const void* a, const void* b, void* out, int64_t n, int op, int dt_a,
                      int dt_b, int dt_out, hipStream_t s) {
    constexpr int SMIN = SA < SB ? (SA < SO ? SA : SO) : (SB < SO ? SB : SO);
    constexpr int V = 16 / SMIN, U = kArElems / V;
    constexpr int kAligned = SO == SMIN ? 2 : (SA == SMIN ? 0 : 1);
    ArArgs g;
    g.a = static_cast<const uint8_t*>(a);
    g.b = static_cast<const uint8_t*>(b);
    g.out = static_cast<uint8_t*>(out);
    g.n = n;
    g.op = op; g.dt_a = dt_a; g.dt_b = dt_b; g.dt_out = dt_out;
    // the aligned stream decides the head (its pointer is element aligned)
    const uintptr_t ap = (uintptr_t)(kAligned == 2 ? out : kAligned == 0 ? a : b);
    int64_t head = (int64_t)((16 - (ap & 15)) & 15) / SMIN;
    if (head > n) head = n;
    g.head = (int32_t)head;
    g.nvec = (n - head) / V;
    // at most one resident round of workgroups, and at most arithmetic_max_blocks()
    int64_t cap = arithmetic_max_blocks();
    static const int resident = resident_blocks(arithmetic_kernel<SA, SB, SO>);  // asked once
    if (resident > 0 && resident < cap) cap = resident;
    const int64_t step_vecs = (int64_t)kArThreads * U;
    int64_t grid = (g.nvec + step_vecs - 1) / step_vecs;
    if (grid > cap) grid = cap;
    if (grid < 1) grid = 1;  // the head and the tail
    hipLaunchKernelGGL((arithmetic_kernel<SA, SB, SO>), dim3((unsigned)grid), dim3(kArThreads), 0,
                       s, g);
    return hipGetLastError();
}

template <int SA, int SB>
hipError_t launch_so(const void* a, const void* b, void* out, int64_t n, int op, int dt_a,
                     int dt_b, int dt_out, hipStream_t s) {
    switch ((int)dtype_size(dt_out)) {
    case 1: return launch_one<SA, SB, 1>(a, b, out, n, op, dt_a, dt_b, dt_out, s);
    case 2: return launch_one<SA, SB, 2>(a, b, out, n, op, dt_a, dt_b, dt_out, s);
    case 4: return launch_one<SA, SB, 4>(a, b, out, n, op, dt_a, dt_b, dt_out, s);
    case 8: return launch_one<SA, SB, 8>(a, b, out, n, op, dt_a, dt_b, dt_out, s);
    default: return hipErrorInvalidValue;
    }
}

template <int SA>
hipError_t launch_sb(const void* a, const void* b, void* out, int64_t n, int op, int dt_a,
                     int dt_b, int dt_out, hipStream_t s) {
    switch ((int)dtype_size(dt_b)) {
    case 1: return launch_so<SA, 1>(a, b, out, n, op, dt_a, dt_b, dt_out, s);
    case 2: return launch_so<SA, 2>(a, b, out, n, op, dt_a, dt_b, dt_out, s);
    case 4: return launch_so<SA, 4>(a, b, out, n, op, dt_a, dt_b, dt_out, s);
    case 8: return launch_so<SA, 8>(a, b, out, n, op, dt_a, dt_b, dt_out, s);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace

int arithmetic_max_blocks() {
    // as pointwise_max_blocks(); ZT_AR_MAX_BLOCKS lowers it (tests reach the grid-stride loop's
    // second trip with a small array)
    if (const char* e = std::getenv("ZT_AR_MAX_BLOCKS")) {
        const long v = std::atol(e);
        if (v >= 1 && v <= 65535) return (int)v;
    }
    return 2048;
}

hipError_t launch_arithmetic(const void* a, int dt_a, const void* b, int dt_b, void* out,
                             int dt_out, int64_t n, int op, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (op < 0 || op >= kArOps) return hipErrorInvalidValue;
    switch ((int)dtype_size(dt_a)) {
    case 1: return launch_sb<1>(a, b, out, n, op, dt_a, dt_b, dt_out, s);
    case 2: return launch_sb<2>(a, b, out, n, op, dt_a, dt_b, dt_out, s);
    case 4: return launch_sb<4>(a, b, out, n, op, dt_a, dt_b, dt_out, s);
    case 8: return launch_sb<8>(a, b, out, n, op, dt_a, dt_b, dt_out, s);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace zt
