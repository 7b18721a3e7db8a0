// pointwise.hip — the per-element filters (reencode, crop, rescale, clamp, equal, replace_value;
// src/filter/filters/{reencode,crop,rescale,clamp,equal,replace_value}.rs) as one kernel that
// evaluates a program of 1..8 ops on every element of an N-d box: strided source (a crop is a
// sub-box), contiguous destination, every element read once and written once.
//
// Values travel through the program widened to a class that Rust `as` commutes with
// (sign- / zero-extend then truncate; a half type converts through f32; half -> f64 is exact):
//   integers of up to 32 bits as i32 / u32, 64-bit integers as i64 / u64, bf16 / f16 / f32 as
//   their exact f32 value, f64 as f64.
// So `as` is written once per (class, output type) on top of as_cast (zt_device.hpp), not once
// per type pair, and every intermediate `as` of a fused program is performed: the result is
// bit-identical to running the ops one launch at a time.
//
// The program is a kernel argument: wave-uniform, read with scalar loads, its branches uniform.
// Each lane carries 16 elements per step in registers, as vectors of EV = 16 / min(input size,
// output size) elements: the side with the smaller element is accessed as one aligned 16-byte
// vector per lane, the other side as EV * size / 16 vectors at element alignment (gfx950 global
// accesses in unaligned mode). The first and last vector of a row that are cut by the row's ends
// go element by element.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdlib>

#include "zt_device.hpp"
#include "zt_kernels.hpp"

namespace zt {

namespace {

constexpr int kPwThreads = 256;
constexpr int kPwElems = 16;  // elements a lane carries per step

__host__ __device__ inline int pw_class_of(int dt) {
    switch (dt) {
    case kI8: case kI16: case kI32: return kPwI32;
    case kI64: return kPwI64;
    case kU64: return kPwU64;
    case kBF16: case kF16: case kF32: return kPwF32;
    case kF64: return kPwF64;
    default: return kPwU32;  // bool, u8, u16, u32
    }
}

// E values of one lane: the class value's bits, low and high words (32-bit classes use lo only).
template <int E>
struct Vals {
    uint32_t lo[E];
    uint32_t hi[E];
};

template <typename C, int E>
__device__ __forceinline__ C vget(const Vals<E>& v, int e) {
    if constexpr (sizeof(C) == 4) return __builtin_bit_cast(C, v.lo[e]);
    else return __builtin_bit_cast(C, ((uint64_t)v.hi[e] << 32) | v.lo[e]);
}
template <typename C, int E>
__device__ __forceinline__ void vset(Vals<E>& v, int e, C c) {
    if constexpr (sizeof(C) == 4) {
        v.lo[e] = __builtin_bit_cast(uint32_t, c);
    } else {
        const uint64_t u = __builtin_bit_cast(uint64_t, c);
        v.lo[e] = (uint32_t)u;
        v.hi[e] = (uint32_t)(u >> 32);
    }
}

// element type -> its class value
__device__ __forceinline__ int32_t widen(int8_t x) { return x; }
__device__ __forceinline__ int32_t widen(int16_t x) { return x; }
__device__ __forceinline__ int32_t widen(int32_t x) { return x; }
__device__ __forceinline__ int64_t widen(int64_t x) { return x; }
__device__ __forceinline__ uint32_t widen(uint8_t x) { return x; }
__device__ __forceinline__ uint32_t widen(uint16_t x) { return x; }
__device__ __forceinline__ uint32_t widen(uint32_t x) { return x; }
__device__ __forceinline__ uint64_t widen(uint64_t x) { return x; }
__device__ __forceinline__ float widen(bf16_t x) { return bf16_bits_to_f32(x.bits); }
__device__ __forceinline__ float widen(f16_t x) { return f16_bits_to_f32(x.bits); }
__device__ __forceinline__ float widen(float x) { return x; }
__device__ __forceinline__ double widen(double x) { return x; }

// `as` from the class C to the element type `dt`, the result widened to dt's class
template <typename C, typename TO, int E>
__device__ __forceinline__ void cast_to(Vals<E>& v) {
#pragma unroll
    for (int e = 0; e < E; ++e) vset(v, e, widen(as_cast<C, TO>(vget<C>(v, e))));
}

template <typename C, int E>
__device__ __forceinline__ void cast_from(Vals<E>& v, int dt) {
    ZT_DISPATCH_DTYPE(dt, TO, (cast_to<C, TO>(v)))
}

template <int E>
__device__ __forceinline__ void cast_all(Vals<E>& v, int cls, int dt) {
    switch (cls) {
    case kPwI32: cast_from<int32_t>(v, dt); break;
    case kPwU32: cast_from<uint32_t>(v, dt); break;
    case kPwI64: cast_from<int64_t>(v, dt); break;
    case kPwU64: cast_from<uint64_t>(v, dt); break;
    case kPwF32: cast_from<float>(v, dt); break;
    default: cast_from<double>(v, dt); break;
    }
}

// `v as f64` (rescale.rs:92, :119): exact from every class but the 64-bit integers (RNE)
template <int E>
__device__ __forceinline__ void to_f64_all(Vals<E>& v, int cls) {
#define ZT_PW_TO_F64(C)                                                                          \
    _Pragma("unroll") for (int e = 0; e < E; ++e) vset(v, e, (double)vget<C>(v, e));
    switch (cls) {
    case kPwI32: ZT_PW_TO_F64(int32_t) break;
    case kPwU32: ZT_PW_TO_F64(uint32_t) break;
    case kPwI64: ZT_PW_TO_F64(int64_t) break;
    case kPwU64: ZT_PW_TO_F64(uint64_t) break;
    case kPwF32: ZT_PW_TO_F64(float) break;
    default: break;
    }
#undef ZT_PW_TO_F64
}

// num_traits::clamp (clamp.rs:150): a NaN element fails both comparisons and passes; a NaN
// bound disables its side.
template <typename C, int E>
__device__ __forceinline__ void clamp_as(Vals<E>& v, uint64_t a, uint64_t b) {
    Vals<1> t;
    t.lo[0] = (uint32_t)a; t.hi[0] = (uint32_t)(a >> 32);
    const C lo = vget<C>(t, 0);
    t.lo[0] = (uint32_t)b; t.hi[0] = (uint32_t)(b >> 32);
    const C hi = vget<C>(t, 0);
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const C x = vget<C>(v, e);
        vset(v, e, x < lo ? lo : (x > hi ? hi : x));
    }
}

// bit e = (element e == value), compared as values of the class: -0.0 == 0.0, NaN equals
// nothing, 64-bit integers compared exactly (equal.rs:62-77, replace_value.rs:82-97)
template <typename C, int E>
__device__ __forceinline__ uint32_t equal_as(const Vals<E>& v, uint64_t a) {
    Vals<1> t;
    t.lo[0] = (uint32_t)a; t.hi[0] = (uint32_t)(a >> 32);
    const C value = vget<C>(t, 0);
    uint32_t m = 0;
#pragma unroll
    for (int e = 0; e < E; ++e) m |= (vget<C>(v, e) == value ? 1u : 0u) << e;
    return m;
}

#define ZT_PW_BY_CLASS(CLS, CALL)                                                                \
    switch (CLS) {                                                                               \
    case kPwI32: { using C = int32_t; CALL; } break;                                             \
    case kPwU32: { using C = uint32_t; CALL; } break;                                            \
    case kPwI64: { using C = int64_t; CALL; } break;                                             \
    case kPwU64: { using C = uint64_t; CALL; } break;                                            \
    case kPwF32: { using C = float; CALL; } break;                                               \
    default: { using C = double; CALL; } break;                                                  \
    }

// A uniform pointer the compiler must take as new: what is loaded through it is loaded where it
// is used, not hoisted and kept in SGPRs across the whole loop body (the kernel arguments are
// read again with scalar loads instead, which is what keeps the SGPR file from spilling).
template <typename P>
__device__ __forceinline__ P fresh(P p) {
    asm volatile("" : "+s"(p));
    return p;
}

// The program on E elements held as storage bits of prog->dt_in on entry (zero-extended) and
// as storage bits of the last op's type on return. `prog` points into the kernel arguments.
template <int ISZ, int OSZ, int E, typename P>
__device__ __forceinline__ void run_program(Vals<E>& v, P prog) {
    // decode: storage bits -> class value
    if constexpr (ISZ == 1) {
        if (prog->dt_in == kI8) {
#pragma unroll
            for (int e = 0; e < E; ++e) v.lo[e] = (uint32_t)(int32_t)(int8_t)v.lo[e];
        }
    } else if constexpr (ISZ == 2) {
        if (prog->dt_in == kI16) {
#pragma unroll
            for (int e = 0; e < E; ++e) v.lo[e] = (uint32_t)(int32_t)(int16_t)v.lo[e];
        } else if (prog->dt_in == kF16) {
#pragma unroll
            for (int e = 0; e < E; ++e) v.lo[e] = f2u(f16_bits_to_f32((uint16_t)v.lo[e]));
        } else if (prog->dt_in == kBF16) {
#pragma unroll
            for (int e = 0; e < E; ++e) v.lo[e] <<= 16;
        }
    }
    int dt = prog->dt_in;
#pragma nounroll
    for (int k = 0; k < prog->n_ops; ++k) {
        const auto* op = &fresh(prog)->ops[k];
        const int kind = op->kind, dt_out = op->dt_out;
        int cls = pw_class_of(dt);
        uint32_t mask = 0;
        bool cast = dt != dt_out;  // the same type: `as` is the identity
        if (kind == kPwRescale) {
            to_f64_all(v, cls);
            cls = kPwF64;
            cast = dt_out != kF64;
            const double mul = __builtin_bit_cast(double, op->a);
            const double add = __builtin_bit_cast(double, op->b);
            if (op->flags & kPwAddFirst) {  // (x + add) * multiply: two roundings (rescale.rs:92)
#pragma unroll
                for (int e = 0; e < E; ++e) vset(v, e, (vget<double>(v, e) + add) * mul);
            } else {  // x.mul_add(multiply, add): one rounding (rescale.rs:119)
#pragma unroll
                for (int e = 0; e < E; ++e) vset(v, e, __builtin_fma(vget<double>(v, e), mul, add));
            }
        } else if (kind == kPwClamp) {
            ZT_PW_BY_CLASS(cls, (clamp_as<C>(v, op->a, op->b)))
        } else if (kind == kPwEqual || kind == kPwReplace) {
            ZT_PW_BY_CLASS(cls, (mask = equal_as<C>(v, op->a)))
        }
        if (kind == kPwEqual) {  // (v == value) as bool / u8
#pragma unroll
            for (int e = 0; e < E; ++e) v.lo[e] = (mask >> e) & 1u;
        } else {
            if (cast) cast_all(v, cls, dt_out);
            if (kind == kPwReplace) {  // `replace` holds the class value of dt_out
                const uint64_t b = fresh(prog)->ops[k].b;
#pragma unroll
                for (int e = 0; e < E; ++e)
                    if ((mask >> e) & 1u) {
                        v.lo[e] = (uint32_t)b;
                        v.hi[e] = (uint32_t)(b >> 32);
                    }
            }
        }
        dt = dt_out;
    }
    // encode: class value -> storage bits
    if constexpr (OSZ == 1) {
#pragma unroll
        for (int e = 0; e < E; ++e) v.lo[e] &= 0xFFu;
    } else if constexpr (OSZ == 2) {
        if (dt == kF16) {
#pragma unroll
            for (int e = 0; e < E; ++e) v.lo[e] = f32_to_f16_bits(u2f(v.lo[e]));
        } else if (dt == kBF16) {
#pragma unroll
            for (int e = 0; e < E; ++e) v.lo[e] = f32_to_bf16_bits(u2f(v.lo[e]));
        } else {
#pragma unroll
            for (int e = 0; e < E; ++e) v.lo[e] &= 0xFFFFu;
        }
    }
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

// N elements of SZ bytes at p (vectors at alignment A) -> zero-extended storage bits, into the
// elements [b, b + N) of v
template <int SZ, int A, int N, int E>
__device__ __forceinline__ void load_wide(const uint8_t* p, Vals<E>& v, int b) {
    constexpr int NV = N * SZ / 16, PER = 16 / SZ;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const Vec16<A> q = *reinterpret_cast<const Vec16<A>*>(p + 16 * i);
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int e = b + i * PER + j;
            if constexpr (SZ == 1) v.lo[e] = (q.w[j / 4] >> (8 * (j % 4))) & 0xFFu;
            else if constexpr (SZ == 2) v.lo[e] = (q.w[j / 2] >> (16 * (j % 2))) & 0xFFFFu;
            else if constexpr (SZ == 4) v.lo[e] = q.w[j];
            else { v.lo[e] = q.w[2 * j]; v.hi[e] = q.w[2 * j + 1]; }
        }
    }
}

template <int SZ, int A, int N, int E>
__device__ __forceinline__ void store_wide(uint8_t* p, const Vals<E>& v, int b) {
    constexpr int NV = N * SZ / 16, PER = 16 / SZ;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        Vec16<A> q;
#pragma unroll
        for (int w = 0; w < 4; ++w) q.w[w] = 0;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int e = b + i * PER + j;
            if constexpr (SZ == 1) q.w[j / 4] |= v.lo[e] << (8 * (j % 4));
            else if constexpr (SZ == 2) q.w[j / 2] |= v.lo[e] << (16 * (j % 2));
            else if constexpr (SZ == 4) q.w[j] = v.lo[e];
            else { q.w[2 * j] = v.lo[e]; q.w[2 * j + 1] = v.hi[e]; }
        }
        *reinterpret_cast<Vec16<A>*>(p + 16 * i) = q;
    }
}

// The kernel's arguments as one block, so that the kernel can read them where it needs them
// through the kernarg segment pointer (scalar loads) instead of holding them all in SGPRs.
struct PwArgs {
    const uint8_t* in;
    uint8_t* out;
    PwGeom g;
    PwProgram prog;
};
typedef const PwArgs __attribute__((address_space(4))) * PwArgsPtr;

// One launch: rows of g.row_len elements, cut into vectors of EV = 16 / min(ISZ, OSZ) elements:
// vector j of a row holds its elements [first + j * EV, first + (j + 1) * EV), with `first` <= 0
// chosen per row so that every vector starts on a 16-byte boundary of the side with the smaller
// element (the output when the sizes are equal). G lanes share a row (256 / G rows per
// workgroup step); a lane's step is U = 16 / EV vectors, G apart, and the program once on 16
// elements. A wave whose lanes' vectors all lie inside their rows (every wave but those at a
// row's ends) takes the interior path: U 16-byte loads issued together, U 16-byte stores, no
// per-vector branch; the other waves go vector by vector, whole vectors as 16-byte accesses
// and cut vectors element by element.
// Workgroup steps (row group, segment of G * U vectors) are grid-strided.
template <int ISZ, int OSZ>
__global__ __launch_bounds__(kPwThreads) void pointwise_kernel(const PwArgs args) {
    constexpr int EV = 16 / (ISZ < OSZ ? ISZ : OSZ);
    constexpr int U = kPwElems / EV, E = kPwElems;
    constexpr bool kAlignOut = OSZ <= ISZ;
    constexpr int AI = kAlignOut ? ISZ : 16, AO = kAlignOut ? 16 : OSZ;
    using TIS = typename Store<ISZ>::type;
    using TOS = typename Store<OSZ>::type;
    const PwArgsPtr kp0 = (PwArgsPtr)__builtin_amdgcn_kernarg_segment_ptr();
    // this workgroup's first step, then (rg, seg) advance by the grid size
    int64_t rg = (int64_t)blockIdx.x / kp0->g.segs, seg = (int64_t)blockIdx.x % kp0->g.segs;
    for (;;) {
        PwArgsPtr kp = fresh(kp0);
        if (rg >= kp->g.row_groups) break;
        const int lg = kp->g.log2_g;
        const int lane = (int)threadIdx.x & ((1 << lg) - 1);
        const int64_t row = ((rg * kPwThreads) >> lg) + ((int)threadIdx.x >> lg);
        // this lane's vectors: jb + u * G, u in [0, U)
        const int64_t jb = ((seg * U) << lg) + lane;
        Vals<E> v;
#pragma unroll
        for (int e = 0; e < E; ++e) { v.lo[e] = 0; v.hi[e] = 0; }
        const uint8_t* src = kp->in;
        uint8_t* dst = kp->out;
        int64_t first = 0, len = 0;  // len = 0: no element of this lane's is inside a row
        if (row < kp->g.rows) {
            // the row's first source element
            int64_t off = kp->g.base;
            const int n_outer = kp->g.n_outer;
            if (n_outer > 0) {
                if (kp->g.rows32) {
                    uint32_t r = (uint32_t)row;
                    for (int d = n_outer - 1; d >= 0; --d) {
                        const uint32_t n = (uint32_t)kp->g.shape[d], q = r / n;
                        off += (int64_t)(r - q * n) * kp->g.stride[d];
                        r = q;
                    }
                } else {
                    int64_t r = row;
                    for (int d = n_outer - 1; d >= 0; --d) {
                        const int64_t n = kp->g.shape[d], q = r / n;
                        off += (r - q * n) * kp->g.stride[d];
                        r = q;
                    }
                }
            }
            len = kp->g.row_len;
            src += off * ISZ;
            dst += row * len * OSZ;
            const uintptr_t ap = kAlignOut ? (uintptr_t)dst : (uintptr_t)src;
            const int64_t h = (int64_t)((16 - (ap & 15)) & 15) / (kAlignOut ? OSZ : ISZ);
            first = h > 0 ? h - EV : 0;
        }
        // element of the lane's vector u: e0(u) = ebase + u * estep
        const int64_t ebase = first + jb * EV, estep = (int64_t)EV << lg;
        const bool inside = ebase >= 0 && ebase + (U - 1) * estep + EV <= len;
        const bool interior = __builtin_amdgcn_ballot_w64(!inside) == 0;  // wave-uniform
        if (interior) {
#pragma unroll
            for (int u = 0; u < U; ++u)
                load_wide<ISZ, AI, EV>(src + (ebase + u * estep) * ISZ, v, u * EV);
        } else {
            // (an address the compiler cannot match with the interior path's, or it splits that
            // path's 16-byte accesses to share their last dword with this one)
            const TIS* srow = reinterpret_cast<const TIS*>(src);
            asm volatile("" : "+v"(srow));
#pragma unroll
            for (int u = 0; u < U; ++u) {
                // [k0, k1) of the vector's elements lie inside the row
                const int64_t e0 = ebase + u * estep;
                if (e0 >= 0 && e0 + EV <= len) {  // a whole vector of a wave at a row's end
                    load_wide<ISZ, AI, EV>(src + e0 * ISZ, v, u * EV);
                    continue;
                }
                const int k0 = e0 < 0 ? (int)-e0 : 0;
                const int k1 = len - e0 < EV ? (len > e0 ? (int)(len - e0) : 0) : EV;
#pragma unroll
                for (int e = 0; e < EV; ++e) {
                    if (e >= k0 && e < k1) {
                        const TIS s = srow[e0 + e];
                        v.lo[u * EV + e] = (uint32_t)s;
                        if constexpr (ISZ == 8) v.hi[u * EV + e] = (uint32_t)(s >> 32);
                    }
                }
            }
        }
        run_program<ISZ, OSZ>(v, &fresh(kp0)->prog);
        if (interior) {
#pragma unroll
            for (int u = 0; u < U; ++u)
                store_wide<OSZ, AO, EV>(dst + (ebase + u * estep) * OSZ, v, u * EV);
        } else {
            TOS* drow = reinterpret_cast<TOS*>(dst);
            asm volatile("" : "+v"(drow));
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t e0 = ebase + u * estep;
                if (e0 >= 0 && e0 + EV <= len) {
                    store_wide<OSZ, AO, EV>(dst + e0 * OSZ, v, u * EV);
                    continue;
                }
                const int k0 = e0 < 0 ? (int)-e0 : 0;
                const int k1 = len - e0 < EV ? (len > e0 ? (int)(len - e0) : 0) : EV;
#pragma unroll
                for (int e = 0; e < EV; ++e) {
                    if (e >= k0 && e < k1) {
                        const int i = u * EV + e;
                        TOS* o = drow + (e0 + e);
                        if constexpr (OSZ == 8) *o = ((uint64_t)v.hi[i] << 32) | v.lo[i];
                        else *o = (TOS)v.lo[i];
                    }
                }
            }
        }
        kp = fresh(kp0);
        rg += kp->g.step_rg;
        seg += kp->g.step_seg;
        if (seg >= kp->g.segs) {
            seg -= kp->g.segs;
            ++rg;
        }
    }
}

// The most workgroups of a kernel the device holds at once: a grid-strided launch of more leaves
// a partly filled last round (at 5 waves per SIMD, 2048 workgroups would run as one full round
// of 1280 and one of 768). 0 if the runtime cannot tell.
template <typename K>
int resident_blocks(K kernel) {
    int dev = 0, cus = 0, per_cu = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kPwThreads, 0) !=
            hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return cus * per_cu;
}

template <int ISZ, int OSZ>
hipError_t launch_one(const void* in, void* out, PwGeom g, const PwProgram& p, hipStream_t s) {
    // at most one resident round of workgroups, and at most pointwise_max_blocks()
    int64_t cap = pointwise_max_blocks();
    static const int resident = resident_blocks(pointwise_kernel<ISZ, OSZ>);  // asked once
    if (resident > 0 && resident < cap) cap = resident;
    int64_t grid = cap;  // items = row_groups * segs, without overflow
    if (g.row_groups <= cap && g.segs <= cap) grid = g.row_groups * g.segs;
    if (grid > cap) grid = cap;
    g.step_rg = grid / g.segs;
    g.step_seg = grid % g.segs;
    PwArgs args;
    args.in = static_cast<const uint8_t*>(in);
    args.out = static_cast<uint8_t*>(out);
    args.g = g;
    args.prog = p;
    hipLaunchKernelGGL((pointwise_kernel<ISZ, OSZ>), dim3((unsigned)grid), dim3(kPwThreads), 0, s,
                       args);
    return hipGetLastError();
}

template <int ISZ>
hipError_t launch_osz(const void* in, void* out, int osz, const PwGeom& g, const PwProgram& p,
                      hipStream_t s) {
    switch (osz) {
    case 1: return launch_one<ISZ, 1>(in, out, g, p, s);
    case 2: return launch_one<ISZ, 2>(in, out, g, p, s);
    case 4: return launch_one<ISZ, 4>(in, out, g, p, s);
    case 8: return launch_one<ISZ, 8>(in, out, g, p, s);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace

int pointwise_max_blocks() {
    // about 8 workgroups of 256 threads per CU: enough to fill the chip, few enough that the
    // launch does not queue tens of thousands of them; ZT_PW_MAX_BLOCKS lowers it (tests reach
    // the grid-stride loop's second trip with a small array)
    if (const char* e = std::getenv("ZT_PW_MAX_BLOCKS")) {
        const long v = std::atol(e);
        if (v >= 1 && v <= 65535) return (int)v;
    }
    return 2048;
}

hipError_t launch_pointwise(const void* in, void* out, PwGeom g, const PwProgram& prog,
                            hipStream_t s) {
    if (g.rows <= 0 || g.row_len <= 0) return hipSuccess;
    if (prog.n_ops < 1 || prog.n_ops > kPwMaxOps) return hipErrorInvalidValue;
    const int dt_out = prog.ops[prog.n_ops - 1].dt_out;
    const int isz = (int)dtype_size(prog.dt_in), osz = (int)dtype_size(dt_out);
    const int EV = 16 / (isz < osz ? isz : osz), U = kPwElems / EV;
    // vectors of a row, the cut first one included; G lanes per row, a power of two, U vectors
    // per lane and step
    const int64_t nv = (g.row_len + 2 * EV - 2) / EV, per_lane = (nv + U - 1) / U;
    int lg = 0;
    while ((1 << lg) < kPwThreads && ((int64_t)1 << lg) < per_lane) ++lg;
    g.log2_g = lg;
    g.segs = (nv + ((int64_t)U << lg) - 1) / ((int64_t)U << lg);
    const int64_t rpb = kPwThreads >> lg;
    g.row_groups = (g.rows + rpb - 1) / rpb;
    g.rows32 = g.rows < ((int64_t)1 << 32) ? 1 : 0;
    switch (isz) {
    case 1: return launch_osz<1>(in, out, osz, g, prog, s);
    case 2: return launch_osz<2>(in, out, osz, g, prog, s);
    case 4: return launch_osz<4>(in, out, osz, g, prog, s);
    case 8: return launch_osz<8>(in, out, osz, g, prog, s);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace zt
