// gradient.hip — gradient magnitude (gradient_magnitude.rs:109-147, kernel.rs:75-129).
//
// Two 3-tap passes along an axis, both with replicate edges at the block bounds:
//   triangle   T: out[k] = (in[max(k-1,0)] * 0.25 + in[k] * 0.5) + in[min(k+1,n-1)] * 0.25
//   difference D: out[k] = 0.5 * (in[min(k+1,n-1)] - in[max(k-1,0)])
// Sobel: for each axis a, the passes i = 0..nd-1 in axis order (D on a, T elsewhere), then
// g += s * s, axes ascending; CentralDifference: s = D_a(input). Result sqrt(g). Every operation is
// an f32 operation of the reference, in its order (no FMA: -ffp-contract=off), so results are
// bit-identical.
//
// 3-D Sobel runs in one z-march per (y, x) tile (gm_sobel3_kernel); every other rank, and
// CentralDifference, run the literal pass-by-pass algorithm on f32 scratch (gm_pass_kernel,
// gm_accumulate_kernel, gm_finish_kernel).

#include <hip/hip_runtime.h>

#include <stdint.h>

#include <algorithm>
#include <type_traits>

#include "zt_device.hpp"
#include "zt_gpu.hpp"
#include "zt_kernels.hpp"

namespace zt {

// V: float, or a pair of floats f2 (gfx950's packed f32 multiply / add: the same IEEE operations on
// two values per instruction; the fused march is bound by its vector arithmetic)
template <typename V>
__device__ __forceinline__ V gm_tri(V a, V b, V c) {
    return (a * 0.25f + b * 0.5f) + c * 0.25f;  // kernel.rs:96-99
}
template <typename V>
__device__ __forceinline__ V gm_diff(V prev, V next) {
    return 0.5f * (next - prev);  // kernel.rs:123-125
}

// ---------------------------------------------------------------------------------------------
// Fused 3-D Sobel. A workgroup owns a 32 x 64 output tile of the (y, x) plane and a segment of
// output slices. It stages the tile plus a 1-element apron (34 rows x 72 columns from x0 - 4:
// whole 4-element quads, columns 0..2 and 69..71 loaded, never read) at coordinates clamped into
// the block (clamping composes across the passes: a pass at a clamped row / column is the pass
// of that row / column). Each thread keeps its staged points' three input slices z-1, z, z+1
// (z clamped) in registers, the next entering slice prefetched a step ahead. Per output slice:
//   tz = Tz v, dz = Dz v at every staged point -> LDS (two buffers, one barrier per step; a
//   row holds element e of its 18 quads at [18 e, 18 e + 18): the 16 lanes of a tile row then
//   read consecutive words and a wave's four row pairs, 144 words apart, distinct banks; with
//   quads stored whole, lanes 4 words apart used a quarter of the banks and 68 % of the LDS
//   cycles were bank conflicts);
//   a thread's 2 rows x 4 columns of outputs: A = Ty dz, B = Dy tz, C = Ty tz on 6 columns,
//   Gz = Tx A, Gy = Tx B, Gx = Dx C, out = sqrt((Gz * Gz + Gy * Gy) + Gx * Gx).
// Every input slice is read once per tile (34 x 72 / (32 x 64) = 1.20 of the tile loaded, 1.10
// used; a segment re-reads two slices to prime its ring), the output written once.
// QUAD (block x extent and region x origin multiples of 4, aligned base, 1/2/4-byte elements):
// each staged quad is one 4/8/16-byte load at its start clamped to [0, nx - 4]; a quad wholly
// left / right of the block then holds the edge element at position 0 / 3, broadcast when the
// slice enters the ring. Otherwise element by element at x clamped to the block. Every address
// comes from coordinates clamped into the block.
// ---------------------------------------------------------------------------------------------
constexpr int kGMTy = 32, kGMTx = 64, kGMNT = 256;
constexpr int kGMTH = kGMTy + 2, kGMMG = 4, kGMTP = kGMTx + 2 * kGMMG, kGMNQX = kGMTP / 4;
constexpr int kGMNQ = kGMTH * kGMNQX, kGMNPQ = (kGMNQ + kGMNT - 1) / kGMNT;
static_assert(kGMTy * kGMTx == 8 * kGMNT, "a thread makes 2 rows x 4 columns of outputs");

// 4 consecutive elements from one 16/8/4-byte load (4/2/1-byte types)
template <typename T>
__device__ __forceinline__ void gm_load4(const T* p, float (&v)[4]) {
    using U = typename UIntOf<sizeof(T)>::type;
    U w[4];
    load4_bits(reinterpret_cast<const U*>(p), w);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = Elem<T>::to_f32(__builtin_bit_cast(T, w[e]));
}

template <typename TIn, bool QUAD>
__global__ __launch_bounds__(kGMNT) void gm_sobel3_kernel(const TIn* __restrict__ in,
                                                          float* __restrict__ out, GMSobel3 p,
                                                          int tiles_x, int tiles_y, int zseg) {
    constexpr int TY = kGMTy, TX = kGMTx, NT = kGMNT, TH = kGMTH, TP = kGMTP, MG = kGMMG;
    constexpr int NQX = kGMNQX, NQ = kGMNQ, NPQ = kGMNPQ;
    __shared__ __attribute__((aligned(16))) float tzb[2][TH * TP];
    __shared__ __attribute__((aligned(16))) float dzb[2][TH * TP];
    const int tid = threadIdx.x;
    const int64_t nz = p.n[0], ny = p.n[1], nx = p.n[2];
    const int64_t onz = p.on[0], ony = p.on[1], onx = p.on[2];
    // XCD-aware block -> (tile, z segment): consecutive logical ids (x-adjacent tiles of one
    // segment) share an XCD, so their aprons come from that XCD's L2
    const int nwg = gridDim.x, b = blockIdx.x;
    const int lid = (nwg % 8 == 0) ? (b % 8) * (nwg / 8) + b / 8 : b;
    const int ntiles = tiles_x * tiles_y;
    const int tile_i = lid % ntiles, seg = lid / ntiles;
    const int64_t x0 = (int64_t)(tile_i % tiles_x) * TX, y0 = (int64_t)(tile_i / tiles_x) * TY;
    const int64_t kz0 = (int64_t)seg * zseg, kz1 = kz0 + zseg < onz ? kz0 + zseg : onz;
    const int hy = (int)(ony - y0 < TY ? ony - y0 : TY);
    const int hx = (int)(onx - x0 < TX ? onx - x0 : TX);
    const int64_t qy0 = p.o0[1] + y0 - 1, qx4 = p.o0[2] + x0 - MG;  // staged tile origin
    const int64_t plane = ny * nx;
    // stores: whole quads when the region width and the base keep them inside and aligned
    const bool quads = (onx % 4 == 0) && (((uintptr_t)out & 15) == 0);

    constexpr int NOFF = QUAD ? NPQ : 4 * NPQ;
    int off[NOFF];  // element offsets in the plane (rows clamped; x clamped per quad / element)
    const bool edgex = qx4 < 0 || qx4 + TP > nx;  // block-uniform
    int bl = 0, br = 0;  // QUAD: bit k = quad k lies wholly left / right of the block
    int wb[NPQ];         // LDS index of quad k's element 0
#pragma unroll
    for (int k = 0; k < NPQ; ++k) {
        const int q = tid + NT * k;
        const int r = q / NQX, cq = q - r * NQX;
        wb[k] = r * TP + cq;
        int64_t qy = qy0 + (r < TH ? r : TH - 1);  // quads past the tile: a valid row, not kept
        qy = qy < 0 ? 0 : (qy > ny - 1 ? ny - 1 : qy);
        if constexpr (QUAD) {
            int64_t xs = qx4 + 4 * cq;
            bl |= xs < 0 ? 1 << k : 0;
            br |= xs > nx - 4 ? 1 << k : 0;
            xs = xs < 0 ? 0 : (xs > nx - 4 ? nx - 4 : xs);
            off[k] = (int)(qy * nx + xs);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                int64_t qx = qx4 + 4 * cq + e;
                qx = qx < 0 ? 0 : (qx > nx - 1 ? nx - 1 : qx);
                off[4 * k + e] = (int)(qy * nx + qx);
            }
        }
    }
    // a staged quad is two pairs of x neighbours (packed f32 arithmetic)
    auto ld = [&](int64_t zq, f2 (&v)[NPQ][2]) {  // input slice zq (clamped to the block)
        zq = zq < 0 ? 0 : (zq > nz - 1 ? nz - 1 : zq);
        const TIn* sl = in + zq * plane;
#pragma unroll
        for (int k = 0; k < NPQ; ++k) {
            float w[4];
            if constexpr (QUAD) {
                gm_load4<TIn>(sl + off[k], w);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) w[e] = Elem<TIn>::to_f32(sl[off[4 * k + e]]);
            }
            v[k][0] = f2{w[0], w[1]};
            v[k][1] = f2{w[2], w[3]};
        }
    };
    auto fix = [&](f2 (&v)[NPQ][2]) {  // edge quads: the edge element broadcast
        if constexpr (QUAD) {
            if (edgex) {
#pragma unroll
                for (int k = 0; k < NPQ; ++k) {
                    const bool l = (bl >> k) & 1, rr = (br >> k) & 1;
                    const float e = l ? v[k][0].x : v[k][1].y;
                    if (l || rr) v[k][0] = v[k][1] = f2{e, e};
                }
            }
        }
    };

    f2 vm[NPQ][2], vc[NPQ][2], vp[NPQ][2], pre[NPQ][2];
    const int64_t zc0 = p.o0[0] + kz0;  // block slice of the segment's first output
    ld(zc0 - 1, vm);
    fix(vm);
    ld(zc0, vc);
    fix(vc);
    ld(zc0 + 1, pre);
    const int r0 = 2 * (tid / 16), c0 = 4 * (tid % 16);  // this thread's outputs in the tile
    for (int64_t kz = kz0; kz < kz1; ++kz) {
#pragma unroll
        for (int k = 0; k < NPQ; ++k)
#pragma unroll
            for (int h = 0; h < 2; ++h) vp[k][h] = pre[k][h];
        fix(vp);
        ld(p.o0[0] + kz + 2, pre);  // next step's entering slice (clamped; unused past the end)
        const int buf = (int)((kz - kz0) & 1);
        float* tzw = tzb[buf];
        float* dzw = dzb[buf];
#pragma unroll
        for (int k = 0; k < NPQ; ++k) {
            f2 t2[2], d2[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                t2[h] = gm_tri(vm[k][h], vc[k][h], vp[k][h]);
                d2[h] = gm_diff(vm[k][h], vp[k][h]);
            }
            const int q = tid + NT * k;
            if (k < NPQ - 1 || q < NQ) {
                const float t4[4] = {t2[0].x, t2[0].y, t2[1].x, t2[1].y};
                const float d4[4] = {d2[0].x, d2[0].y, d2[1].x, d2[1].y};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    tzw[wb[k] + e * NQX] = t4[e];
                    dzw[wb[k] + e * NQX] = d4[e];
                }
            }
        }
        // one barrier per step: this step's reads of buffer `buf` end before any thread passes
        // the next step's barrier, and only the step after that writes `buf` again
        lds_barrier();
        // staged rows r0 .. r0 + 3, window columns i = 0..5 = staged columns c0 + 3 .. c0 + 8
        // (output column c = staged column c + MG): element 3 of the thread's quad c0 / 4, the
        // quad after it, element 0 of the next; held as the pairs (1,2), (3,4), (0,5)
        constexpr int CO[6] = {3 * NQX, 1, NQX + 1, 2 * NQX + 1, 3 * NQX + 1, 2};
        constexpr int CA[3] = {1, 3, 0}, CB[3] = {2, 4, 5};
        f2 t[4][3], d[4][3];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float* tr = tzw + (r0 + j) * TP + c0 / 4;
            const float* dr = dzw + (r0 + j) * TP + c0 / 4;
#pragma unroll
            for (int pi = 0; pi < 3; ++pi) {
                t[j][pi] = f2{tr[CO[CA[pi]]], tr[CO[CB[pi]]]};
                d[j][pi] = f2{dr[CO[CA[pi]]], dr[CO[CB[pi]]]};
            }
        }
        // y passes on column pairs, then each column's two rows paired for the x passes
        f2 Ar[6], Br[6], Cr[6];
        {
            f2 A[2][3], B[2][3], C[2][3];
#pragma unroll
            for (int rr = 0; rr < 2; ++rr)
#pragma unroll
                for (int pi = 0; pi < 3; ++pi) {
                    A[rr][pi] = gm_tri(d[rr][pi], d[rr + 1][pi], d[rr + 2][pi]);  // Ty Dz v
                    B[rr][pi] = gm_diff(t[rr][pi], t[rr + 2][pi]);                // Dy Tz v
                    C[rr][pi] = gm_tri(t[rr][pi], t[rr + 1][pi], t[rr + 2][pi]);  // Ty Tz v
                }
#pragma unroll
            for (int pi = 0; pi < 3; ++pi) {
                Ar[CA[pi]] = f2{A[0][pi].x, A[1][pi].x};
                Ar[CB[pi]] = f2{A[0][pi].y, A[1][pi].y};
                Br[CA[pi]] = f2{B[0][pi].x, B[1][pi].x};
                Br[CB[pi]] = f2{B[0][pi].y, B[1][pi].y};
                Cr[CA[pi]] = f2{C[0][pi].x, C[1][pi].x};
                Cr[CB[pi]] = f2{C[0][pi].y, C[1][pi].y};
            }
        }
        float o4[2][4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const f2 gz = gm_tri(Ar[c], Ar[c + 1], Ar[c + 2]);  // axis 0
            const f2 gy = gm_tri(Br[c], Br[c + 1], Br[c + 2]);  // axis 1
            const f2 gx = gm_diff(Cr[c], Cr[c + 2]);            // axis 2
            f2 g = gz * gz;  // 0 + s * s == s * s
            g = g + gy * gy;
            g = g + gx * gx;
            o4[0][c] = sqrtf(g.x);
            o4[1][c] = sqrtf(g.y);
        }
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
            const int r = r0 + rr;
            if (r < hy && c0 < hx) {
                float* dst = out + (kz * ony + y0 + r) * onx + x0 + c0;
                if (quads) {  // onx % 4 == 0: a started quad lies inside the row
                    *reinterpret_cast<float4*>(dst) =
                        make_float4(o4[rr][0], o4[rr][1], o4[rr][2], o4[rr][3]);
                } else {
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        if (c0 + c < hx) dst[c] = o4[rr][c];
                }
            }
        }
#pragma unroll
        for (int k = 0; k < NPQ; ++k)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                vm[k][h] = vc[k][h];
                vc[k][h] = vp[k][h];
            }
    }
}

int gm_sobel3_zseg(const GMSobel3& p, int64_t* nseg_out) {
    const int64_t tiles =
        ((p.on[1] + kGMTy - 1) / kGMTy) * ((p.on[2] + kGMTx - 1) / kGMTx);
    // z segments: about two rounds of full occupancy over the launch, at least kGMSegMin output
    // slices each (a segment re-reads two slices to prime its ring)
    const int64_t per_launch = 2 * 256 * 4;
    const int64_t want = (per_launch + tiles - 1) / std::max<int64_t>(tiles, 1);
    int64_t nseg = std::max<int64_t>(
        1, std::min<int64_t>(want, (p.on[0] + kGMSegMin - 1) / kGMSegMin));
    const int64_t zseg = (p.on[0] + nseg - 1) / nseg;
    nseg = (p.on[0] + zseg - 1) / zseg;
    if (nseg_out) *nseg_out = nseg;
    return (int)zseg;
}

bool gm_sobel3_supported(const GMSobel3& p) {
    // planes addressed by 32-bit element offsets; the grid's x dimension holds every workgroup
    if (p.n[1] * p.n[2] >= 0x7FFFFFFF || p.on[0] > 0x7FFFFFFF) return false;
    const int64_t tx = (p.on[2] + kGMTx - 1) / kGMTx, ty = (p.on[1] + kGMTy - 1) / kGMTy;
    if (tx > 0xFFFFFF || ty > 0xFFFFFF) return false;
    const int64_t nseg = (p.on[0] + kGMSegMin - 1) / kGMSegMin;  // upper bound
    return tx * ty <= 0x7FFFFFFF / std::max<int64_t>(nseg, 1);
}

hipError_t launch_gm_sobel3(const void* in, int dtype_in, float* out, const GMSobel3& p,
                            hipStream_t s) {
    if (p.on[0] * p.on[1] * p.on[2] == 0) return hipSuccess;
    if (!gm_sobel3_supported(p)) return hipErrorInvalidValue;
    const int tiles_x = (int)((p.on[2] + kGMTx - 1) / kGMTx);
    const int tiles_y = (int)((p.on[1] + kGMTy - 1) / kGMTy);
    int64_t nseg = 1;
    const int zseg = gm_sobel3_zseg(p, &nseg);
    const dim3 grid((unsigned)((int64_t)tiles_x * tiles_y * nseg));
    const int esz = (int)dtype_size(dtype_in);
    // quads need a 4-aligned x origin and extent and an aligned base
    const bool quad = p.n[2] % 4 == 0 && p.n[2] >= 4 && p.o0[2] % 4 == 0 &&
                      (uintptr_t)in % (4 * (uintptr_t)esz) == 0;
    hipError_t err = hipErrorInvalidValue;
    ZT_DISPATCH_DTYPE(dtype_in, T,
        // (quad instantiations for the common element types only: build time)
        if constexpr (std::is_same_v<T, float> || std::is_same_v<T, uint16_t> ||
                      std::is_same_v<T, uint8_t>) {
            if (quad)
                hipLaunchKernelGGL((gm_sobel3_kernel<T, true>), grid, dim3(kGMNT), 0, s,
                                   static_cast<const T*>(in), out, p, tiles_x, tiles_y, zseg);
            else
                hipLaunchKernelGGL((gm_sobel3_kernel<T, false>), grid, dim3(kGMNT), 0, s,
                                   static_cast<const T*>(in), out, p, tiles_x, tiles_y, zseg);
        } else {
            hipLaunchKernelGGL((gm_sobel3_kernel<T, false>), grid, dim3(kGMNT), 0, s,
                               static_cast<const T*>(in), out, p, tiles_x, tiles_y, zseg);
        }
        err = hipGetLastError())
    return err;
}

// ---------------------------------------------------------------------------------------------
// Generic N-d path: the reference's passes one by one on the whole block.
// ---------------------------------------------------------------------------------------------

// T or D along one axis of a C-order block seen as outer x n x inner
template <typename TIn, bool DIFF>
__global__ __launch_bounds__(256) void gm_pass_kernel(const TIn* __restrict__ in,
                                                      float* __restrict__ out, int64_t total,
                                                      int64_t n, int64_t inner) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t k = (i / inner) % n;
        const int64_t kp = k > 0 ? k - 1 : 0, kn = k + 1 < n ? k + 1 : n - 1;
        const float prev = Elem<TIn>::to_f32(in[i + (kp - k) * inner]);
        const float next = Elem<TIn>::to_f32(in[i + (kn - k) * inner]);
        if constexpr (DIFF) out[i] = gm_diff(prev, next);
        else out[i] = gm_tri(prev, Elem<TIn>::to_f32(in[i]), next);
    }
}

__global__ __launch_bounds__(256) void gm_accumulate_kernel(float* __restrict__ g,
                                                            const float* __restrict__ s,
                                                            int64_t total, bool first) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        const float v = s[i];
        g[i] = (first ? 0.0f : g[i]) + v * v;  // *g += s * s from zeros
    }
}

// sqrt, extract_subset and the `as` cast: out (C order, out_shape) from the block's g
template <typename TOut>
__global__ __launch_bounds__(256) void gm_finish_kernel(const float* __restrict__ g,
                                                        TOut* __restrict__ out, NdGeom geom) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < geom.out_numel;
         i += (int64_t)gridDim.x * blockDim.x) {
        int64_t rem = i, src = 0, stride = 1;
        for (int d = geom.ndim - 1; d >= 0; --d) {
            const int64_t c = rem % geom.out_shape[d];
            rem /= geom.out_shape[d];
            src += (geom.out_start[d] + c) * stride;
            stride *= geom.shape[d];
        }
        out[i] = from_f32<TOut>(sqrtf(g[src]));
    }
}

static int gm_grid(int64_t n) {
    const int64_t b = (n + 255) / 256;
    return (int)(b > 256 * 64 ? 256 * 64 : (b < 1 ? 1 : b));
}

hipError_t launch_gm_pass(const void* in, int dtype_in, float* out, int64_t outer, int64_t n,
                          int64_t inner, bool diff, hipStream_t s) {
    const int64_t total = outer * n * inner;
    if (total == 0) return hipSuccess;
    hipError_t err = hipErrorInvalidValue;
    ZT_DISPATCH_DTYPE(dtype_in, T,
        if (diff)
            hipLaunchKernelGGL((gm_pass_kernel<T, true>), dim3(gm_grid(total)), dim3(256), 0, s,
                               static_cast<const T*>(in), out, total, n, inner);
        else
            hipLaunchKernelGGL((gm_pass_kernel<T, false>), dim3(gm_grid(total)), dim3(256), 0, s,
                               static_cast<const T*>(in), out, total, n, inner);
        err = hipGetLastError())
    return err;
}

hipError_t launch_gm_accumulate(float* g, const float* sq, int64_t total, bool first,
                                hipStream_t s) {
    if (total == 0) return hipSuccess;
    hipLaunchKernelGGL(gm_accumulate_kernel, dim3(gm_grid(total)), dim3(256), 0, s, g, sq, total,
                       first);
    return hipGetLastError();
}

hipError_t launch_gm_finish(const float* g, int dtype_out, void* out, const NdGeom& geom,
                            hipStream_t s) {
    if (geom.out_numel == 0) return hipSuccess;
    hipError_t err = hipErrorInvalidValue;
    ZT_DISPATCH_DTYPE(dtype_out, T,
        hipLaunchKernelGGL(gm_finish_kernel<T>, dim3(gm_grid(geom.out_numel)), dim3(256), 0, s, g,
                           static_cast<T*>(out), geom);
        err = hipGetLastError())
    return err;
}

}  // namespace zt
