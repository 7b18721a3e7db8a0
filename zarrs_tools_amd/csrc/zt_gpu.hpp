// zt_gpu.hpp — the device helpers that the kernels share, one definition of each (DESIGN.md
// §3). Device-only: included by the .hip files and by gf_fused.hpp. Tile constants, tuning
// #defines and anything only one kernel uses stay in that kernel's file.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include <type_traits>

#include "zt_kernels.hpp"

namespace zt {

// Compile-time loop: f(integral_constant<I>) for I in [B, E).
template <int B, int E, typename F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (B < E) {
        f(std::integral_constant<int, B>{});
        static_for<B + 1, E>(f);
    }
}

// Workgroup barrier for LDS hand-offs only. __syncthreads() also fences global memory, which
// makes the compiler drain every outstanding global load (vmcnt(0)), including the loads a
// march keeps in flight across the barrier: this one leaves the prefetch in flight (the
// compiler still waits for it at its first use). A hand-off through global memory must not
// use it.
__device__ __forceinline__ void lds_barrier() {
    __asm__ volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// ---- buffer (SRD) access: a slice's base goes in a descriptor, each point keeps a 32-bit byte
//      offset, and the hardware range check makes an offset past num_records read 0 / drop the
//      store. So out-of-block points need no 64-bit address math and no branch around a memory
//      instruction, and the compiler's vmcnt accounting waits for exactly the step-old prefetch
//      instead of draining every load.
using rsrc_t = __amdgpu_buffer_rsrc_t;
constexpr int kBadOff = (int)0x80000000;  // >= num_records of any slice: reads 0, writes drop

// Build descriptors only from kernel arguments and loop counters (wave-uniform scalars), so
// hipcc keeps them in SGPRs: no readfirstlane, no waterfall loops.
__device__ __forceinline__ rsrc_t make_rsrc(const void* base, uint32_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), (short)0, (int)bytes,
                                             0x00020000);
}

// One f32 at a byte offset.
template <int AUX = 0>
__device__ __forceinline__ float load_f32(rsrc_t r, int off) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, off, 0, AUX));
}

// Hide a value from the optimiser: keeps `ok ? off : kBadOff` a v_cndmask feeding one
// unconditional buffer access (otherwise the select becomes an exec-masked branch around two
// accesses, and the compiler's vmcnt accounting across the branch drains the loads in flight).
__device__ __forceinline__ int opaque(int v) {
    __asm__ volatile("" : "+v"(v));
    return v;
}

// Packed pair of f32 (v_pk_add_f32 / v_pk_mul_f32 / v_pk_fma_f32: both lanes for one issue).
typedef float f2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ f2 pk_fma(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }

// Elements of the radius-r window at i that lie inside [0, n).
__device__ __forceinline__ int clamped_count(int i, int n, int r) {
    int lo = i - r < 0 ? 0 : i - r;
    int hi = i + r > n - 1 ? n - 1 : i + r;
    return hi - lo + 1;
}

// x / d for an integer count d given rcp = RN(1/d): Markstein's correction step makes the
// quotient correctly rounded (checked exhaustively-by-sampling for d <= 70000, tools/README),
// so this equals IEEE division at 3 VALU ops instead of ~11.
__device__ __forceinline__ float div_by_count(float x, float d, float rcp) {
    float q = x * rcp;
    float r = __builtin_fmaf(-q, d, x);
    return __builtin_fmaf(r, rcp, q);
}

// v_rcp_f32 flushes subnormals on both sides: the reciprocal of a d above 2^126 comes back as 0
// (fast_div would return 0 where the quotient is near 1), that of a subnormal d as inf (NaN
// after the correction). True for such a result (zero, subnormal or infinite), so one
// v_cmp_class_f32 on the reciprocal tells whether d is inside [2^-126, 2^126].
__device__ __forceinline__ bool rcp_unusable(float y) {
    return __builtin_amdgcn_class(y, 0x2F4);  // -inf, -sub, -0, +0, +sub, +inf
}

// s / (s + eps): rcp + one Newton step + Markstein correction (6 VALU ops instead of the ~12 of
// IEEE division; within 1 ulp, almost always correctly rounded). Special values follow IEEE:
// 0/0 and inf/inf give NaN as in the reference. A d outside [2^-126, 2^126] (rcp_unusable)
// takes the IEEE division, in a branch that tame data never enters.
__device__ __forceinline__ float fast_div(float x, float d) {
    float y = __builtin_amdgcn_rcpf(d);
    if (__builtin_expect(rcp_unusable(y), 0)) return x / d;
    float e = __builtin_fmaf(-d, y, 1.0f);
    y = __builtin_fmaf(e, y, y);
    float q = x * y;
    float r = __builtin_fmaf(-d, q, x);
    return __builtin_fmaf(r, y, q);
}

// The unsigned integer type of ESZ bytes: an element's storage bits.
template <int ESZ> struct UIntOf {
    static_assert(ESZ == 1 || ESZ == 2 || ESZ == 4 || ESZ == 8, "element sizes of 1/2/4/8 bytes");
    using type = std::conditional_t<ESZ == 1, uint8_t,
                 std::conditional_t<ESZ == 2, uint16_t,
                 std::conditional_t<ESZ == 4, uint32_t, uint64_t>>>;
};

// 4 consecutive elements' storage bits out of the 16/8/4 bytes q that hold them (4/2/1-byte
// elements; q a 4-vector, a 2-vector or one uint32_t).
template <typename K, typename Q>
__device__ __forceinline__ void unpack4(const Q& q, K (&v)[4]) {
    if constexpr (sizeof(K) == 4) {
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else if constexpr (sizeof(K) == 2) {
        v[0] = (K)(q.x & 0xffffu), v[1] = (K)(q.x >> 16);
        v[2] = (K)(q.y & 0xffffu), v[3] = (K)(q.y >> 16);
    } else {
        static_assert(sizeof(K) == 1, "quad loads of 1/2/4-byte elements");
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (K)((q >> (8 * e)) & 0xffu);
    }
}
// The same from one load at p, which is aligned to the 4 elements.
template <typename K>
__device__ __forceinline__ void load4_bits(const K* p, K (&v)[4]) {
    if constexpr (sizeof(K) == 4) unpack4(*reinterpret_cast<const uint4*>(p), v);
    else if constexpr (sizeof(K) == 2) unpack4(*reinterpret_cast<const uint2*>(p), v);
    else unpack4(*reinterpret_cast<const uint32_t*>(p), v);
}

// Least / greatest of two keys.
template <typename K> __device__ __forceinline__ K kmin(K a, K b) { return a < b ? a : b; }
template <typename K> __device__ __forceinline__ K kmax(K a, K b) { return a > b ? a : b; }

// storage bits <-> order key of width K; mode: kRankKeyUnsigned / Signed / Float (floats: bits ^
// (sign ? all ones : sign bit), signed integers: bits ^ sign bit, the others as they are), so
// unsigned compares of keys order the elements. comp = all ones reverses the order.
template <typename K>
__device__ __forceinline__ K to_order_key(K b, int mode, K comp = 0) {
    constexpr K S = (K)((K)1 << (8 * sizeof(K) - 1));
    const K f = (b & S) ? (K)~(K)0 : S;
    return (K)(b ^ (mode == kRankKeyFloat ? f : (mode == kRankKeySigned ? S : (K)0)) ^ comp);
}
template <typename K>
__device__ __forceinline__ K from_order_key(K k, int mode, K comp = 0) {
    constexpr K S = (K)((K)1 << (8 * sizeof(K) - 1));
    k = (K)(k ^ comp);
    const K f = (k & S) ? S : (K)~(K)0;
    return (K)(k ^ (mode == kRankKeyFloat ? f : (mode == kRankKeySigned ? S : (K)0)));
}

}  // namespace zt
