// rank.hip — the neighbourhood rank filters: minimum, median, maximum.
//
// Output k selects one element of the window in[clamp(k_a + i_a, 0, n_a - 1)], i_a in
// [-h_a, h_a] on every axis (replicate edges at the block bounds): the smallest, the one of rank
// (N - 1) / 2, or the largest under a total order. The kernels never do arithmetic on elements:
// an element's storage bits become an unsigned key at the load (floats: bits ^ (sign ? all ones :
// sign bit), signed integers: bits ^ sign bit, unsigned and bool: the bits), the selection uses
// unsigned compares, and the selected key becomes storage bits again at the store. The float key
// orders -NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN; payloads pass through.
//
//   rank3_kernel        3-D, h = (1, 1, 1), 1/2/4-byte elements: one z-march per (y, x) tile
//   rank_pass_kernel    minimum / maximum along one axis (they separate per axis), any rank / h
//   rank_median_kernel  median by bisection over the key's bits, any rank, any h with N <= 4096

#include <hip/hip_runtime.h>

#include <stdint.h>

#include <algorithm>

#include "zt_device.hpp"
#include "zt_gpu.hpp"
#include "zt_kernels.hpp"

namespace zt {

// to_order_key / from_order_key (zt_gpu.hpp) on a key widened to 32 bits, for the fused kernel:
// with S the sign bit of the W-bit element, xs = S for signed and float elements (else 0) and
// xf = S - 1 for float elements (else 0), both made on the host: key = b ^ xs ^ (b negative ? xf
// : 0), and the same two steps in the other order turn a key back (the sign of key ^ xs is the
// element's sign).
template <int W>
__device__ __forceinline__ uint32_t rk_key32(uint32_t b, uint32_t xs, uint32_t xf) {
    return b ^ xs ^ ((uint32_t)((int32_t)(b << (32 - W)) >> 31) & xf);
}
template <int W>
__device__ __forceinline__ uint32_t rk_unkey32(uint32_t k, uint32_t xs, uint32_t xf) {
    const uint32_t t = k ^ xs;
    return t ^ ((uint32_t)((int32_t)(t << (32 - W)) >> 31) & xf);
}

__device__ __forceinline__ uint32_t rk_min3(uint32_t a, uint32_t b, uint32_t c) {
    return kmin(kmin(a, b), c);
}
__device__ __forceinline__ uint32_t rk_max3(uint32_t a, uint32_t b, uint32_t c) {
    return kmax(kmax(a, b), c);
}
__device__ __forceinline__ uint32_t rk_med3(uint32_t a, uint32_t b, uint32_t c) {
    return kmax(kmin(a, b), kmin(kmax(a, b), c));
}
__device__ __forceinline__ void rk_cx(uint32_t& a, uint32_t& b) {  // compare-exchange
    const uint32_t lo = kmin(a, b), hi = kmax(a, b);
    a = lo;
    b = hi;
}

// Forgetful selection of the median of 27: of S live values the smallest moves to a[0] and the
// largest to a[S - 1]; neither can be the median of all 27 while S - 1 >= the count that has to
// lie on one side of it, so both are forgotten, the next value enters and S - 1 values stay.
// From S = 15 down to 4 that is 12 rounds and the 12 values w[15..26]; the median of the last 3
// is the answer. A round of S values takes S / 2 exchanges that order the pairs (i, S - 1 - i),
// then (S + 1) / 2 - 1 to bring the minimum of the lower half (and the middle) down and
// S - 1 - S / 2 to bring the maximum of the upper half (and the middle) up: 144 exchanges over
// the 12 rounds, 288 min / max and 4 for the last three.
template <int S>
__device__ __forceinline__ void rk_min_max_to_ends(uint32_t (&a)[15]) {
#pragma unroll
    for (int i = 0; i < S / 2; ++i) rk_cx(a[i], a[S - 1 - i]);
#pragma unroll
    for (int i = 1; i < (S + 1) / 2; ++i) rk_cx(a[0], a[i]);
#pragma unroll
    for (int i = S / 2; i < S - 1; ++i) rk_cx(a[i], a[S - 1]);
}
template <int S>
__device__ __forceinline__ void rk_forget(uint32_t (&a)[15], const uint32_t (&w)[27]) {
    if constexpr (S > 3) {
        rk_min_max_to_ends<S>(a);
        a[0] = w[30 - S];  // a[S - 1] leaves
        rk_forget<S - 1>(a, w);
    }
}
__device__ __forceinline__ uint32_t rk_median27(const uint32_t (&w)[27]) {
    uint32_t a[15];
#pragma unroll
    for (int i = 0; i < 15; ++i) a[i] = w[i];
    rk_forget<15>(a, w);
    return rk_med3(a[0], a[1], a[2]);
}

// ---------------------------------------------------------------------------------------------
// Fused 3-D kernel, h = (1, 1, 1): gm_sobel3_kernel's data flow. A workgroup owns a 32 x 64 tile
// of the (y, x) plane of the output region and a segment of output slices. It stages the tile
// plus a 1-element apron (34 rows x 72 columns from x0 - 4: whole 4-element quads, columns 0..2
// and 69..71 loaded, never read) at coordinates clamped into the block, so every address is in
// bounds; a thread keeps its 3 staged quads' slices z - 1, z, z + 1 (z clamped) as u32 keys in
// registers, the entering slices prefetched one step (median) or two steps (minimum / maximum)
// ahead. Per output slice:
//   minimum / maximum: the z reduction of every staged point -> LDS (two buffers, one barrier
//     per step); a thread then reduces 10 rows x 3 columns along x and 8 outputs along y;
//   median: every staged point's z triple sorted (3 exchanges, shared by the 9 windows that hold
//     the column) -> three LDS planes (one buffer, two barriers per step); a thread selects rank
//     13 of its 9 sorted triples (rk_median27) for 8 rows of one column, rolling three rows of 9
//     keys in registers.
// A thread's column is tid % 64, so a wave reads 64 consecutive LDS words of a row (no bank
// conflict) and stores 64 consecutive elements.
// ---------------------------------------------------------------------------------------------
constexpr int kRKTy = 32, kRKTx = 64, kRKNT = 256;
constexpr int kRKTH = kRKTy + 2, kRKMG = 4, kRKTW = kRKTx + 2 * kRKMG, kRKNS = kRKTH * kRKTW;
constexpr int kRKNQX = kRKTW / 4, kRKNQ = kRKTH * kRKNQX;
constexpr int kRKNPQ = (kRKNQ + kRKNT - 1) / kRKNT;  // staged quads per thread
constexpr int kRKNP = 4 * kRKNPQ;                    // staged points per thread
constexpr int kRKRows = kRKTy * kRKTx / kRKNT;       // output rows per thread
static_assert(kRKNT % kRKTx == 0 && kRKRows * (kRKNT / kRKTx) == kRKTy, "thread -> column strip");

template <typename K, int KIND, bool QUAD>
__global__ __launch_bounds__(kRKNT) void rank3_kernel(const K* __restrict__ in,
                                                      K* __restrict__ out, Rank3 p, int tiles_x,
                                                      int tiles_y, int zseg, uint32_t xs, uint32_t xf) {
    constexpr int W = 8 * (int)sizeof(K);
    constexpr int TY = kRKTy, TX = kRKTx, NT = kRKNT, TH = kRKTH, TW = kRKTW, NS = kRKNS;
    constexpr int MG = kRKMG, NQX = kRKNQX, NQ = kRKNQ, NPQ = kRKNPQ;
    constexpr int NP = kRKNP, NB = KIND == kRankMedian ? 3 : 1;
    // minimum / maximum: two buffers, one barrier per step. The median's three planes in two
    // buffers would leave room for 2 workgroups per CU; its step is long, so it takes one buffer
    // and a second barrier instead.
    constexpr int NBUF = KIND == kRankMedian ? 1 : 2;
    __shared__ __attribute__((aligned(16))) uint32_t lds[NBUF][NB][NS];
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

    constexpr int NOFF = QUAD ? NPQ : NP;
    int off[NOFF];  // element offsets in the plane (rows clamped; x clamped per quad / element)
    const bool edgex = qx4 < 0 || qx4 + TW > nx;  // block-uniform
    int bl = 0, br = 0;  // QUAD: bit k = quad k lies wholly left / right of the block
    int wb[NPQ];         // LDS index of quad k's element 0 (a multiple of 4)
#pragma unroll
    for (int k = 0; k < NPQ; ++k) {
        const int q = tid + NT * k;
        const int r = q / NQX, cq = q - r * NQX;
        wb[k] = r * TW + 4 * cq;
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
    // input slice zq (clamped to the block) as keys. QUAD (block x extent and region x origin
    // multiples of 4, aligned base): a staged quad is one load at its start clamped to
    // [0, nx - 4]; a quad wholly left / right of the block then holds the edge element at
    // position 0 / 3, which is broadcast. Otherwise element by element at x clamped to the block.
    auto ld = [&](int64_t zq, uint32_t (&v)[NP]) {
        zq = zq < 0 ? 0 : (zq > nz - 1 ? nz - 1 : zq);
        const K* sl = in + zq * plane;
#pragma unroll
        for (int k = 0; k < NPQ; ++k) {
            K w[4];
            if constexpr (QUAD) {
                load4_bits<K>(sl + off[k], w);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) w[e] = sl[off[4 * k + e]];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) v[4 * k + e] = rk_key32<W>((uint32_t)w[e], xs, xf);
        }
    };
    auto fix = [&](uint32_t (&v)[NP]) {  // edge quads: the edge element broadcast
        if constexpr (QUAD) {
            if (edgex) {
#pragma unroll
                for (int k = 0; k < NPQ; ++k) {
                    const bool l = (bl >> k) & 1, rr = (br >> k) & 1;
                    const uint32_t e = l ? v[4 * k] : v[4 * k + 3];
                    if (l || rr) v[4 * k] = v[4 * k + 1] = v[4 * k + 2] = v[4 * k + 3] = e;
                }
            }
        }
    };

    // Slices entering the ring are prefetched AHEAD steps before their step. The median's step is
    // long (vector arithmetic): one slice in flight covers the load latency. A minimum / maximum
    // step is short and waits on memory, so it keeps two slices in flight (measured 1.4 % faster
    // on f32, 3 % on u8), in two register buffers that the steps take in turn
    // (no copy of a buffer that a load still targets).
    constexpr int AHEAD = KIND == kRankMedian ? 1 : 2;
    uint32_t vm[NP], vc[NP], vp[NP], pre0[NP], pre1[NP];
    const int64_t zc0 = p.o0[0] + kz0;  // block slice of the segment's first output
    ld(zc0 - 1, vm);
    fix(vm);
    ld(zc0, vc);
    fix(vc);
    ld(zc0 + 1, pre0);
    if constexpr (AHEAD == 2) ld(zc0 + 2, pre1);
    // this thread's column (staged column cx + MG - 1 is its left neighbour) and first row
    const int cx = tid % TX, r0 = kRKRows * (tid / TX);
    // one output slice kz; pre holds its entering slice and is refilled for step kz + AHEAD
    auto step = [&](int64_t kz, int buf, uint32_t (&pre)[NP]) {
#pragma unroll
        for (int k = 0; k < NP; ++k) vp[k] = pre[k];
        fix(vp);
        ld(p.o0[0] + kz + 1 + AHEAD, pre);  // (clamped; unused past the end)
#pragma unroll
        for (int k = 0; k < NPQ; ++k) {
            const int q = tid + NT * k;
            if (k < NPQ - 1 || q < NQ) {
                uint32_t lo[4], mid[4], hi[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int j = 4 * k + e;
                    if constexpr (KIND == kRankMinimum) {
                        lo[e] = rk_min3(vm[j], vc[j], vp[j]);
                    } else if constexpr (KIND == kRankMaximum) {
                        lo[e] = rk_max3(vm[j], vc[j], vp[j]);
                    } else {
                        uint32_t a = vm[j], m = vc[j], c = vp[j];
                        rk_cx(a, m);
                        rk_cx(m, c);
                        rk_cx(a, m);
                        lo[e] = a, mid[e] = m, hi[e] = c;
                    }
                }
                *reinterpret_cast<uint4*>(&lds[buf][0][wb[k]]) =
                    make_uint4(lo[0], lo[1], lo[2], lo[3]);
                if constexpr (KIND == kRankMedian) {
                    *reinterpret_cast<uint4*>(&lds[buf][1][wb[k]]) =
                        make_uint4(mid[0], mid[1], mid[2], mid[3]);
                    *reinterpret_cast<uint4*>(&lds[buf][2][wb[k]]) =
                        make_uint4(hi[0], hi[1], hi[2], hi[3]);
                }
            }
        }
        // two buffers, one barrier per step: this step's reads of buffer `buf` end before any
        // thread passes the next step's barrier, and only the step after that writes `buf` again
        lds_barrier();
        K* dst = out + (kz * ony + y0 + r0) * onx + x0 + cx;
        if constexpr (KIND != kRankMedian) {
            const uint32_t* L = lds[buf][0] + r0 * TW + cx + MG - 1;
            uint32_t h[kRKRows + 2];
#pragma unroll
            for (int j = 0; j < kRKRows + 2; ++j) {
                const uint32_t* row = L + j * TW;
                h[j] = KIND == kRankMinimum ? rk_min3(row[0], row[1], row[2])
                                            : rk_max3(row[0], row[1], row[2]);
            }
#pragma unroll
            for (int i = 0; i < kRKRows; ++i) {
                const uint32_t o = KIND == kRankMinimum ? rk_min3(h[i], h[i + 1], h[i + 2])
                                                        : rk_max3(h[i], h[i + 1], h[i + 2]);
                if (r0 + i < hy && cx < hx) dst[i * onx] = (K)rk_unkey32<W>(o, xs, xf);
            }
        } else {
            // w[0..9), [9..18), [18..27): staged rows r0 + i, + 1, + 2; a row holds its three
            // columns' sorted triples
            uint32_t w[27];
            auto row9 = [&](int r, int at) {
#pragma unroll
                for (int pl = 0; pl < 3; ++pl) {
                    const uint32_t* row = lds[buf][pl] + r * TW + cx + MG - 1;
#pragma unroll
                    for (int c = 0; c < 3; ++c) w[at + 3 * c + pl] = row[c];
                }
            };
            row9(r0, 0);
            row9(r0 + 1, 9);
#pragma unroll 1
            for (int i = 0; i < kRKRows; ++i) {
                row9(r0 + i + 2, 18);
                const uint32_t o = rk_median27(w);
                if (r0 + i < hy && cx < hx) dst[i * onx] = (K)rk_unkey32<W>(o, xs, xf);
#pragma unroll
                for (int j = 0; j < 18; ++j) w[j] = w[j + 9];
            }
            lds_barrier();  // one buffer: every read ends before the next step's writes
        }
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            vm[k] = vc[k];
            vc[k] = vp[k];
        }
    };
    if constexpr (AHEAD == 1) {
        for (int64_t kz = kz0; kz < kz1; ++kz) step(kz, 0, pre0);
    } else {
        for (int64_t kz = kz0; kz < kz1; kz += 2) {
            step(kz, 0, pre0);
            if (kz + 1 < kz1) step(kz + 1, 1, pre1);  // uniform over the workgroup
        }
    }
}

int rank3_zseg(const Rank3& p, int64_t* nseg_out) {
    const int64_t tiles = ((p.on[1] + kRKTy - 1) / kRKTy) * ((p.on[2] + kRKTx - 1) / kRKTx);
    // z segments: about two rounds of full occupancy over the launch, at least kRankSegMin
    // output slices each (a segment re-reads two slices to prime its ring)
    const int64_t per_launch = 2 * 256 * 4;
    const int64_t want = (per_launch + tiles - 1) / std::max<int64_t>(tiles, 1);
    int64_t nseg = std::max<int64_t>(
        1, std::min<int64_t>(want, (p.on[0] + kRankSegMin - 1) / kRankSegMin));
    const int64_t zseg = (p.on[0] + nseg - 1) / nseg;
    nseg = (p.on[0] + zseg - 1) / zseg;
    if (nseg_out) *nseg_out = nseg;
    return (int)zseg;
}

bool rank3_supported(const Rank3& p, int esz) {
    if (esz != 1 && esz != 2 && esz != 4) return false;
    // planes addressed by 32-bit element offsets; the grid's x dimension holds every workgroup
    if (p.n[1] * p.n[2] >= 0x7FFFFFFF || p.on[0] > 0x7FFFFFFF) return false;
    const int64_t tx = (p.on[2] + kRKTx - 1) / kRKTx, ty = (p.on[1] + kRKTy - 1) / kRKTy;
    if (tx > 0xFFFFFF || ty > 0xFFFFFF) return false;
    const int64_t nseg = (p.on[0] + kRankSegMin - 1) / kRankSegMin;  // upper bound
    return tx * ty <= 0x7FFFFFFF / std::max<int64_t>(nseg, 1);
}

template <typename K, bool QUAD>
static hipError_t rank3_launch_kq(const K* i, K* o, const Rank3& p, int kind, int mode, dim3 grid,
                                  int tiles_x, int tiles_y, int zseg, hipStream_t s) {
    const uint32_t sign = 1u << (8 * sizeof(K) - 1);
    const uint32_t xs = mode == kRankKeyUnsigned ? 0u : sign;
    const uint32_t xf = mode == kRankKeyFloat ? sign - 1 : 0u;
    if (kind == kRankMinimum)
        hipLaunchKernelGGL((rank3_kernel<K, kRankMinimum, QUAD>), grid, dim3(kRKNT), 0, s, i, o,
                           p, tiles_x, tiles_y, zseg, xs, xf);
    else if (kind == kRankMaximum)
        hipLaunchKernelGGL((rank3_kernel<K, kRankMaximum, QUAD>), grid, dim3(kRKNT), 0, s, i, o,
                           p, tiles_x, tiles_y, zseg, xs, xf);
    else
        hipLaunchKernelGGL((rank3_kernel<K, kRankMedian, QUAD>), grid, dim3(kRKNT), 0, s, i, o, p,
                           tiles_x, tiles_y, zseg, xs, xf);
    return hipGetLastError();
}

template <typename K>
static hipError_t rank3_launch_k(const void* in, void* out, const Rank3& p, int kind, int mode,
                                 dim3 grid, int tiles_x, int tiles_y, int zseg, hipStream_t s) {
    const K* i = static_cast<const K*>(in);
    K* o = static_cast<K*>(out);
    // quads need a 4-aligned x origin and extent and an aligned base
    const bool quad = p.n[2] % 4 == 0 && p.n[2] >= 4 && p.o0[2] % 4 == 0 &&
                      (uintptr_t)in % (4 * sizeof(K)) == 0;
    return quad ? rank3_launch_kq<K, true>(i, o, p, kind, mode, grid, tiles_x, tiles_y, zseg, s)
                : rank3_launch_kq<K, false>(i, o, p, kind, mode, grid, tiles_x, tiles_y, zseg, s);
}

hipError_t launch_rank3(const void* in, void* out, int esz, int mode, int kind, const Rank3& p,
                        hipStream_t s) {
    if (p.on[0] * p.on[1] * p.on[2] == 0) return hipSuccess;
    if (!rank3_supported(p, esz)) return hipErrorInvalidValue;
    const int tiles_x = (int)((p.on[2] + kRKTx - 1) / kRKTx);
    const int tiles_y = (int)((p.on[1] + kRKTy - 1) / kRKTy);
    int64_t nseg = 1;
    const int zseg = rank3_zseg(p, &nseg);
    const dim3 grid((unsigned)((int64_t)tiles_x * tiles_y * nseg));
    if (esz == 1)
        return rank3_launch_k<uint8_t>(in, out, p, kind, mode, grid, tiles_x, tiles_y, zseg, s);
    if (esz == 2)
        return rank3_launch_k<uint16_t>(in, out, p, kind, mode, grid, tiles_x, tiles_y, zseg, s);
    return rank3_launch_k<uint32_t>(in, out, p, kind, mode, grid, tiles_x, tiles_y, zseg, s);
}

// ---------------------------------------------------------------------------------------------
// Generic minimum / maximum: one pass along the axis of extent n of a C-order block outer x n x
// inner; output k (of `on`) covers the block positions [o0 + k - h, o0 + k + h] cut to
// [0, n - 1] (a replicated edge element is already in the cut window). Consecutive threads take
// consecutive inner positions, so the last axis (inner == 1) is read along the row. An output
// reads its whole cut window: min(2h + 1, n) reads per element, not a running window's constant
// (DESIGN.md §3.11 names the two-scan form as the follow-up for large h).
// ---------------------------------------------------------------------------------------------
template <typename K, bool MAX>
__global__ __launch_bounds__(256) void rank_pass_kernel(const K* __restrict__ in,
                                                        K* __restrict__ out, int64_t total,
                                                        int64_t n, int64_t on, int64_t o0,
                                                        int64_t h, int64_t inner, int mode) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t q = i / inner, c = i - q * inner;
        const int64_t o = q / on, k = q - o * on;
        const int64_t lo = o0 + k - h < 0 ? 0 : o0 + k - h;
        const int64_t hi = o0 + k + h > n - 1 ? n - 1 : o0 + k + h;
        const K* src = in + o * n * inner + c;
        K acc = to_order_key<K>(src[lo * inner], mode);
        for (int64_t j = lo + 1; j <= hi; ++j) {
            const K v = to_order_key<K>(src[j * inner], mode);
            acc = MAX ? (v > acc ? v : acc) : (v < acc ? v : acc);
        }
        out[i] = from_order_key<K>(acc, mode);
    }
}

static int rk_grid(int64_t n) {
    const int64_t b = (n + 255) / 256;
    return (int)(b > 256 * 64 ? 256 * 64 : (b < 1 ? 1 : b));
}

template <typename K>
static hipError_t rank_pass_k(const void* in, void* out, int64_t total, const RankPass& p,
                              bool max, int mode, hipStream_t s) {
    if (max)
        hipLaunchKernelGGL((rank_pass_kernel<K, true>), dim3(rk_grid(total)), dim3(256), 0, s,
                           static_cast<const K*>(in), static_cast<K*>(out), total, p.n, p.on,
                           p.o0, p.h, p.inner, mode);
    else
        hipLaunchKernelGGL((rank_pass_kernel<K, false>), dim3(rk_grid(total)), dim3(256), 0, s,
                           static_cast<const K*>(in), static_cast<K*>(out), total, p.n, p.on,
                           p.o0, p.h, p.inner, mode);
    return hipGetLastError();
}

hipError_t launch_rank_pass(const void* in, void* out, int esz, int mode, bool max,
                            const RankPass& p, hipStream_t s) {
    const int64_t total = p.outer * p.on * p.inner;
    if (total == 0) return hipSuccess;
    if (p.n <= 0 || p.o0 < 0 || p.o0 + p.on > p.n || p.h < 0) return hipErrorInvalidValue;
    switch (esz) {
    case 1: return rank_pass_k<uint8_t>(in, out, total, p, max, mode, s);
    case 2: return rank_pass_k<uint16_t>(in, out, total, p, max, mode, s);
    case 4: return rank_pass_k<uint32_t>(in, out, total, p, max, mode, s);
    case 8: return rank_pass_k<uint64_t>(in, out, total, p, max, mode, s);
    default: return hipErrorInvalidValue;
    }
}

// ---------------------------------------------------------------------------------------------
// Generic median: per output, bisection over the key's bits from the top. With r = (N - 1) / 2,
// the answer is the largest key v with #(window keys < v) <= r; bit by bit, the candidate
// res | bit is kept when that count is <= r. 8 * sizeof(K) x N compares, no per-thread array and
// nothing that depends on N at compile time. The window's rows (every axis but the last) are
// walked by one index that is the same for all threads; the window is read through the cache.
// ---------------------------------------------------------------------------------------------
template <typename K>
__global__ __launch_bounds__(256) void rank_median_kernel(const K* __restrict__ in,
                                                          K* __restrict__ out, RankMedian p,
                                                          int mode) {
    const int nd = p.ndim;
    const int64_t nl = p.shape[nd - 1], hl = p.half[nd - 1];
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < p.out_numel;
         i += (int64_t)gridDim.x * blockDim.x) {
        int64_t c[kMaxDims];  // block coordinates of the output (static indices: registers)
        int64_t rem = i;
#pragma unroll
        for (int d = kMaxDims - 1; d >= 0; --d) {
            c[d] = 0;
            if (d < nd) {
                const int64_t q = rem / p.out_shape[d];
                c[d] = p.out_start[d] + (rem - q * p.out_shape[d]);
                rem = q;
            }
        }
        int64_t cl = 0;  // the last axis' coordinate
#pragma unroll
        for (int d = 0; d < kMaxDims; ++d)
            if (d == nd - 1) cl = c[d];
        const int64_t xlo = cl - hl, xhi = cl + hl;
        K res = 0;
        for (int bit = 8 * (int)sizeof(K) - 1; bit >= 0; --bit) {
            const K cand = (K)(res | ((K)1 << bit));
            int below = 0;
            for (int w = 0; w < p.rows; ++w) {
                int wr = w;  // uniform: the row's offsets on the axes before the last
                int64_t base = 0;
#pragma unroll
                for (int d = kMaxDims - 2; d >= 0; --d) {
                    if (d < nd - 1) {
                        const int win = 2 * (int)p.half[d] + 1;
                        const int q = wr / win;
                        int64_t pos = c[d] + (wr - q * win) - p.half[d];
                        wr = q;
                        pos = pos < 0 ? 0 : (pos > p.shape[d] - 1 ? p.shape[d] - 1 : pos);
                        base += pos * p.stride[d];
                    }
                }
                const K* row = in + base;
                for (int64_t x = xlo; x <= xhi; ++x) {
                    const int64_t xc = x < 0 ? 0 : (x > nl - 1 ? nl - 1 : x);
                    below += to_order_key<K>(row[xc], mode) < cand ? 1 : 0;
                }
            }
            if (below <= p.rank) res = cand;
        }
        out[i] = from_order_key<K>(res, mode);
    }
}

hipError_t launch_rank_median(const void* in, void* out, int esz, int mode, const RankMedian& p,
                              hipStream_t s) {
    if (p.out_numel == 0) return hipSuccess;
    if (p.ndim < 1 || p.ndim > kMaxDims || p.rows < 1) return hipErrorInvalidValue;
    for (int d = 0; d < p.ndim; ++d)
        if (p.shape[d] <= 0 || p.half[d] < 0 || p.out_start[d] < 0 ||
            p.out_start[d] + p.out_shape[d] > p.shape[d])
            return hipErrorInvalidValue;
    const dim3 grid(rk_grid(p.out_numel)), block(256);
    switch (esz) {
    case 1:
        hipLaunchKernelGGL(rank_median_kernel<uint8_t>, grid, block, 0, s,
                           static_cast<const uint8_t*>(in), static_cast<uint8_t*>(out), p, mode);
        break;
    case 2:
        hipLaunchKernelGGL(rank_median_kernel<uint16_t>, grid, block, 0, s,
                           static_cast<const uint16_t*>(in), static_cast<uint16_t*>(out), p,
                           mode);
        break;
    case 4:
        hipLaunchKernelGGL(rank_median_kernel<uint32_t>, grid, block, 0, s,
                           static_cast<const uint32_t*>(in), static_cast<uint32_t*>(out), p,
                           mode);
        break;
    case 8:
        hipLaunchKernelGGL(rank_median_kernel<uint64_t>, grid, block, 0, s,
                           static_cast<const uint64_t*>(in), static_cast<uint64_t*>(out), p,
                           mode);
        break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace zt
