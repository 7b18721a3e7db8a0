// labels.hip — per-label statistics and the label size filter (extensions: the reference has no
// such operation) for gfx950.
//
// A label array holds 0 for background and 1 .. K for objects. The statistics are a reduction keyed
// by label into the state of zt_labels_host.hpp: (K + 1) rows of u64 columns, struct-of-arrays
// (count; per axis smallest, largest and summed coordinate; with an intensity array the smallest
// and largest orderable key and the 128-bit sum), and one trailing word that counts the elements
// outside [0, K]. Every column is an integer sum, minimum or maximum, so the result is unique
// whatever the launch geometry.
//
//   lbl_init_kernel     the identity of every column
//   lbl_stats_kernel    a workgroup owns tiles of kLblTileRows rows x 64 x of the box (rows = every
//                       axis but the last, flattened); a wave takes 64 consecutive x of a row. Rows
//                       that are 16-byte aligned are staged through LDS with 16-byte loads, others
//                       are read element by element. A ballot of "differs from the lane before"
//                       gives every lane the ends of its run of equal labels (clz / ctz of the
//                       masked word); the run's head lane contributes the whole run in closed form:
//                       count = length, x-sum = the arithmetic series, x-min / x-max = the run's
//                       ends, the outer coordinates times the length. Intensities are reduced along
//                       the run by a segmented shuffle reduction of 6 steps. Run results are
//                       combined in an LDS table keyed by label (open addressing, a slot's key
//                       claimed by compare-and-swap, at most kLblProbes probes, LDS atomic add /
//                       min / max) that lives across the workgroup's tiles and is flushed with one
//                       set of 64-bit global atomics per label present when it is half full, after
//                       kLblFlushTiles tiles, and at the end. A run that finds no slot goes to the
//                       global atomics directly. Background costs no atomic. The box, its origin,
//                       the waves' outer coordinates and the per-element constants are held in LDS
//                       and a run's columns are walked with one stride, so that the kernel keeps
//                       within its scalar registers (no spills).
//   lbl_keep_scan_kernel one workgroup: keep[l] = count[l] in [min_size, max_size], the exclusive
//                       prefix of keep, remap[l], the kept count K' and the largest label kept
//   lbl_gather_kernel   out[i] = remap[in[i]]
//
// Termination: every loop is bounded by the tile count, the row length, the probe bound, the slot
// count or K. No kernel waits for another workgroup, spins on a flag or depends on the order
// workgroups run in; the two barriers of a tile are reached by every thread of the workgroup. The
// flush decision compares a counter of claimed slots that only grows (nothing resets it) with its
// value at the last flush; it is read after the tile's second barrier, and no lane adds to it before
// the next tile's first, so every thread decides alike.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdlib>
#include <type_traits>

#include "zt_device.hpp"
#include "zt_gpu.hpp"
#include "zt_kernels.hpp"
#include "zt_labels_host.hpp"

namespace zt {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int T = kLblTileRows;
constexpr int kRowsPerWave = T / kWaves;
constexpr int kLblProbes = 8;
// The table is flushed after this many tiles at the latest: 2^20 tiles * 2^10 elements * 2^32 per
// element keeps a workgroup's intensity partial inside an int64_t.
constexpr uint32_t kLblFlushTiles = 1u << 20;
constexpr int kLblMaxTableBytes = 40 * 1024;
static_assert(T % kWaves == 0, "a wave owns whole rows of a tile");


struct LblGeom {
    int64_t dim[kMaxDims];  // the box, padded in front with unit axes
    int64_t org[kMaxDims];  // its origin in the whole array, padded in front with zeros
    int64_t rows, X, segs, tiles;
    int32_t ndim;  // the rank before padding
};

// The intensity's key, branch-free for every type: key = w ^ ((w & i_fsign) ? i_nflip : i_pflip),
// a NaN when (w & ~i_fsign) > i_inf; the summed value is (w ^ i_sflip) - i_sflip.
//   unsigned: all 0, i_inf all ones;  signed: i_pflip = i_nflip = i_sflip = the sign bit;
//   float formats: i_fsign = i_pflip = the sign bit, i_nflip = every bit, i_inf = the bits of +inf
struct LblArgs {
    uint64_t K;
    uint64_t lab_neg;  // the sign bit of a signed label type, else 0
    int32_t slots;     // LDS slots, a power of two
    int32_t i_sum;     // intensity sums are kept (integers of up to 32 bits)
    uint64_t i_fsign, i_pflip, i_nflip, i_sflip, i_inf;
};

// (64-bit only: a second, 32-bit form of every division costs more scalar registers for its
// hoisted reciprocals than the kernel has)
__device__ __forceinline__ void divmod(uint64_t a, uint64_t b, uint64_t& q, uint64_t& r) {
    q = a / b;
    r = a - q * b;
}

using ull = unsigned long long;

// sum (lo, hi) += p, p an int64_t's bits, modulo 2^128
__device__ __forceinline__ void add128(ull* lo, ull* hi, uint64_t p) {
    if (p == 0) return;
    const uint64_t old = atomicAdd(lo, (ull)p);
    uint64_t h = (p >> 63) ? ~0ull : 0ull;  // the sign extension of a negative partial
    if (old + p < old) h += 1;              // the carry out of the low word
    if (h) atomicAdd(hi, (ull)h);
}

// One run's contribution to the columns of its label, walking from column to column: p is the
// label's word of column 0 and `stride` the words between columns (the LDS table: the slot and the
// slot count; the state: the label and K + 1), so no column needs an address of its own in a
// scalar register. c / org: the row's outer coordinates and the box's origin, indexed from `pad`.
template <bool COUNT, bool INT, bool GLOBAL, typename KI>
__device__ __forceinline__ void lbl_put(ull* p, uint64_t stride, uint64_t len, uint64_t xg,
                                        const uint64_t* c, const uint64_t* org, int pad, KI klo,
                                        KI khi, int64_t isum) {
    atomicAdd(p, (ull)len);
    if constexpr (!COUNT) {
#pragma unroll 1
        for (int k = pad; k < kMaxDims - 1; ++k) {
            const uint64_t cg = org[k] + c[k];
            p += stride;
            atomicMin(p, (ull)cg);
            p += stride;
            atomicMax(p, (ull)cg);
            p += stride;
            atomicAdd(p, (ull)(cg * len));
        }
        p += stride;
        atomicMin(p, (ull)xg);
        p += stride;
        atomicMax(p, (ull)(xg + len - 1));
        p += stride;
        atomicAdd(p, (ull)(len * xg + len * (len - 1) / 2));
        if constexpr (INT) {
            const bool any = klo <= khi;  // the run has a non-NaN element
            p += stride;
            if (any) atomicMin(p, (ull)klo);
            p += stride;
            if (any) atomicMax(p, (ull)khi);
            p += stride;
            if constexpr (GLOBAL) add128(p, p + stride, (uint64_t)isum);
            else if (isum) atomicAdd(p, (ull)isum);
        }
    }
}

__global__ __launch_bounds__(kThreads) void lbl_init_kernel(ull* state, uint64_t K1, int cols,
                                                            int ndim, int count_only) {
    const uint64_t words = (uint64_t)cols * K1 + 1;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < words;
         i += (uint64_t)gridDim.x * kThreads) {
        const int c = (int)(i / K1);
        // minima start as all ones: the axes' (columns 1, 4, ...) and the intensity's
        const bool is_min = !count_only && c >= 1 && c < cols &&
                            (c <= 3 * ndim ? (c - 1) % 3 == 0 : c == 3 * ndim + 1);
        state[i] = is_min ? ~0ull : 0ull;
    }
}

// EL, EI: bytes of a label and of an intensity element (EI = 0: no intensity array).
template <int EL, int EI, bool COUNT>
__global__ __launch_bounds__(kThreads) void lbl_stats_kernel(const uint8_t* __restrict__ lab,
                                                             const uint8_t* __restrict__ inten,
                                                             const LblGeom g, const LblArgs a,
                                                             int vec_l, int vec_i,
                                                             ull* __restrict__ state) {
    using UL = typename UIntOf<EL>::type;
    using UI = typename UIntOf<EI ? EI : 1>::type;
    using KI = std::conditional_t<EI == 8, uint64_t, uint32_t>;
    constexpr bool INT = EI != 0 && !COUNT;
    extern __shared__ __attribute__((aligned(16))) uint8_t s_dyn[];
    __shared__ __attribute__((aligned(16))) uint8_t s_l[T * 64 * EL];
    __shared__ __attribute__((aligned(16))) uint8_t s_i[INT ? T * 64 * EI : 16];
    __shared__ uint32_t s_claimed;
    // the box, its origin and every wave's outer coordinates live in LDS: loops over the axes
    // index them at run time, and nothing of them is held in registers across a tile
    __shared__ uint64_t s_dim[kMaxDims], s_org[kMaxDims], s_c[kWaves][kMaxDims];
    // the per-element constants too: read where used, they live in vector registers
    __shared__ uint64_t s_par[10];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int S = a.slots;
    const int nd = g.ndim, pad = kMaxDims - nd;
    const int cols = COUNT ? 1 : 1 + 3 * nd + (INT ? 4 : 0);
    const int ci = 1 + 3 * nd;  // the first intensity column
    const uint64_t K1 = a.K + 1;
    uint32_t* keys = reinterpret_cast<uint32_t*>(s_dyn);
    ull* tab = reinterpret_cast<ull*>(s_dyn + (((size_t)S * 4 + 7) & ~(size_t)7));

    // a slot's columns, walked S words at a time, back at their identities
    auto reset_slot = [&](int s) {
        keys[s] = 0;
        ull* q = tab + s;
        *q = 0;
        if constexpr (!COUNT) {
#pragma unroll 1
            for (int ax = 0; ax < nd; ++ax) {
                q += S;
                *q = ~0ull;
                q += S;
                *q = 0;
                q += S;
                *q = 0;
            }
            if constexpr (INT) {
                q += S;
                *q = ~0ull;
                q += S;
                *q = 0;
                q += S;
                *q = 0;
            }
        }
    };
    // one set of global atomics per label present, then the slot is empty again
    auto flush = [&]() {
#pragma unroll 1
        for (int s = tid; s < S; s += kThreads) {
            const uint32_t key = keys[s];
            if (key == 0) continue;
            const ull* q = tab + s;
            ull* p = state + key;
            atomicAdd(p, *q);
            if constexpr (!COUNT) {
#pragma unroll 1
                for (int ax = 0; ax < nd; ++ax) {
                    q += S, p += K1;
                    atomicMin(p, *q);
                    q += S, p += K1;
                    atomicMax(p, *q);
                    q += S, p += K1;
                    atomicAdd(p, *q);
                }
                if constexpr (INT) {
                    const ull lo = q[S], hi = q[2 * S];
                    q += 3 * S;
                    p += K1;
                    if (lo <= hi) atomicMin(p, lo);  // the label has a non-NaN element here
                    p += K1;
                    if (lo <= hi) atomicMax(p, hi);
                    p += K1;
                    add128(p, p + K1, *q);
                }
            }
            reset_slot(s);
        }
    };

    for (int s = tid; s < S; s += kThreads) reset_slot(s);
    if (tid == 0) s_claimed = 0;
    if (tid < kMaxDims) {
        s_dim[tid] = (uint64_t)g.dim[tid];
        s_org[tid] = (uint64_t)g.org[tid];
    }
    if (tid == 0) {
        s_par[0] = a.K;
        s_par[1] = a.lab_neg;
        s_par[2] = a.i_fsign;
        s_par[3] = a.i_pflip;
        s_par[4] = a.i_nflip;
        s_par[5] = a.i_sflip;
        s_par[6] = a.i_inf;
        s_par[7] = (uint64_t)g.rows;
        s_par[8] = (uint64_t)g.X;
    }
    __syncthreads();

    uint32_t bad_n = 0, since = 0, claimed0 = 0;
    for (uint64_t t = blockIdx.x; t < (uint64_t)g.tiles; t += gridDim.x) {
        uint64_t rt, seg;
        divmod(t, (uint64_t)g.segs, rt, seg);
        const uint64_t row0 = rt * T, x0 = seg * 64;
        const int nx = (int)(s_par[8] - x0 < 64 ? s_par[8] - x0 : 64);
        const bool vl = vec_l && nx == 64;
        const bool vi = INT && vec_i && nx == 64;

        // 1. aligned rows: 16 bytes per lane into LDS
        if (vl) {
            constexpr int kPieces = 4 * EL;  // 16-byte pieces of a row of the tile
            for (int p = tid; p < T * kPieces; p += kThreads) {
                const uint64_t row = row0 + p / kPieces;
                uint4 v = make_uint4(0, 0, 0, 0);
                if (row < s_par[7])
                    v = *reinterpret_cast<const uint4*>(lab + (row * s_par[8] + x0) * EL +
                                                        (p % kPieces) * 16);
                *reinterpret_cast<uint4*>(s_l + p * 16) = v;
            }
        }
        if constexpr (INT) {
            if (vi) {
                constexpr int kPieces = 4 * EI;
                for (int p = tid; p < T * kPieces; p += kThreads) {
                    const uint64_t row = row0 + p / kPieces;
                    uint4 v = make_uint4(0, 0, 0, 0);
                    if (row < s_par[7])
                        v = *reinterpret_cast<const uint4*>(inten + (row * s_par[8] + x0) * EI +
                                                            (p % kPieces) * 16);
                    *reinterpret_cast<uint4*>(s_i + p * 16) = v;
                }
            }
        }
        __syncthreads();  // A: the staged rows, and the table as the last flush left it

        // 2. the wave's rows: local coordinates of its first row on the outer axes
        // (every lane of the wave computes and stores the same values)
        uint64_t* c = s_c[wave];
        {
            uint64_t r = row0 + (uint64_t)wave * kRowsPerWave;
            for (int k = kMaxDims - 2; k > pad; --k) {
                uint64_t rem;
                divmod(r, s_dim[k], r, rem);
                c[k] = rem;
            }
            if (pad <= kMaxDims - 2) c[pad] = r;
        }
#pragma unroll 1
        for (int j = 0; j < kRowsPerWave; ++j) {
            const int rl = wave * kRowsPerWave + j;
            const uint64_t row = row0 + rl;
            if (row < s_par[7]) {
                const uint64_t e = row * s_par[8] + x0 + lane;  // the lane's element of the box
                uint64_t u = 0;
                if (lane < nx)
                    u = vl ? (uint64_t)reinterpret_cast<const UL*>(s_l)[rl * 64 + lane]
                           : (uint64_t)reinterpret_cast<const UL*>(lab)[e];
                const bool bad = (u & s_par[1]) != 0 || u > s_par[0];
                bad_n += bad;
                const uint32_t l = bad ? 0u : (uint32_t)u;
                if (__ballot(l != 0) != 0) {
                    const uint32_t prev = __shfl_up(l, 1, 64);
                    const uint64_t H = __ballot(lane == 0 || l != prev);  // heads of runs
                    const uint64_t upto = (2ull << lane) - 1;             // lanes 0 .. lane
                    const int start = 63 - __clzll((long long)(H & upto));
                    const uint64_t above = H & ~upto;
                    const int end = above ? __builtin_ctzll(above) - 1 : 63;

                    KI klo = ~(KI)0, khi = 0;
                    int64_t isum = 0;
                    if constexpr (INT) {
                        KI w = 0;
                        if (lane < nx)
                            w = vi ? (KI)reinterpret_cast<const UI*>(s_i)[rl * 64 + lane]
                                   : (KI)reinterpret_cast<const UI*>(inten)[e];
                        const KI fsign = (KI)s_par[2];
                        const KI key = w ^ ((w & fsign) ? (KI)s_par[4] : (KI)s_par[3]);
                        if (lane < nx && (KI)(w & ~fsign) <= (KI)s_par[6]) klo = khi = key;
                        if (a.i_sum)
                            isum = (int64_t)(uint64_t)(KI)(w ^ (KI)s_par[5]) -
                                   (int64_t)s_par[5];
                        // along the run: lane i ends with the reduction of lanes i .. end
#pragma unroll
                        for (int d = 1; d < 64; d <<= 1) {
                            const KI ol = (KI)__shfl_down((std::conditional_t<EI == 8, ull, unsigned>)klo, d, 64);
                            const KI oh = (KI)__shfl_down((std::conditional_t<EI == 8, ull, unsigned>)khi, d, 64);
                            const bool in_run = lane + d <= end;
                            if (in_run) {
                                klo = ol < klo ? ol : klo;
                                khi = oh > khi ? oh : khi;
                            }
                            if (a.i_sum) {
                                const long long os = __shfl_down((long long)isum, d, 64);
                                if (in_run) isum += os;
                            }
                        }
                    }

                    if (l != 0 && lane == start) {  // the head lane owns the run
                        const uint64_t len = (uint64_t)(end - start + 1);
                        const uint64_t xg = s_org[kMaxDims - 1] + x0 + start;
                        int slot = -1;
                        {
                            const uint32_t h = l & (uint32_t)(S - 1);
                            const int probes = S < kLblProbes ? S : kLblProbes;
#pragma unroll 1
                            for (int p = 0; p < probes; ++p) {
                                const int s = (int)((h + p) & (uint32_t)(S - 1));
                                const uint32_t old = atomicCAS(&keys[s], 0u, l);
                                if (old == 0) atomicAdd(&s_claimed, 1u);
                                if (old == 0 || old == l) {
                                    slot = s;
                                    break;
                                }
                            }
                        }
                        if (slot >= 0)
                            lbl_put<COUNT, INT, false, KI>(tab + slot, (uint64_t)S, len, xg, c,
                                                           s_org, pad, klo, khi, isum);
                        else  // no slot within the probe bound: straight to the state
                            lbl_put<COUNT, INT, true, KI>(state + l, K1, len, xg, c, s_org, pad,
                                                          klo, khi, isum);
                    }
                }
            }
            // the next row of the box: an odometer over the outer axes
            for (int k = kMaxDims - 2; k >= pad; --k) {
                const uint64_t v = c[k] + 1;
                if (v == s_dim[k] && k > pad) {
                    c[k] = 0;
                } else {
                    c[k] = v;
                    break;
                }
            }
        }
        __syncthreads();  // B: every run of the tile is in the table
        // s_claimed only grows (nothing resets it) and no lane adds to it between B and the next
        // A, so every thread reads the same value here; `since` and `claimed0` (the counter at the
        // last flush) are per-thread copies of the same numbers: the decision is uniform
        const uint32_t claimed = s_claimed;
        ++since;
        if (2 * (claimed - claimed0) > (uint32_t)S || since >= kLblFlushTiles) {
            flush();
            since = 0;
            claimed0 = claimed;
        }
    }
    __syncthreads();
    flush();
    if (bad_n) atomicAdd(&state[(uint64_t)cols * K1], (ull)bad_n);
}

// ---- the size filter ---------------------------------------------------------------------------

constexpr int kScanThreads = 1024, kScanPer = 8;

// remap[l] for l in 0 .. K from the counts; kept[0] = K', kept[1] = the largest label kept. One
// workgroup.
__global__ __launch_bounds__(kScanThreads) void lbl_keep_scan_kernel(
    const ull* __restrict__ count, uint64_t K, uint64_t min_size, uint64_t max_size, int relabel,
    uint32_t* __restrict__ remap, uint64_t* kept) {
    __shared__ uint64_t s_wave[kScanThreads / 64];
    __shared__ ull s_largest;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_largest = 0;
    uint64_t carry = 0, largest = 0;
    for (uint64_t c0 = 0; c0 <= K; c0 += kScanThreads * kScanPer) {
        const uint64_t e0 = c0 + (uint64_t)tid * kScanPer;
        uint32_t keep = 0, sum = 0;
#pragma unroll
        for (int q = 0; q < kScanPer; ++q) {
            const uint64_t l = e0 + q;
            const uint64_t n = l >= 1 && l <= K ? count[l] : 0;
            const bool k = n >= min_size && n <= max_size;  // min_size >= 1: absent labels go
            keep |= (uint32_t)k << q;
            sum += k;
            if (k) largest = l;
        }
        unsigned incl = sum;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned o = __shfl_up(incl, off, 64);
            if (lane >= off) incl += o;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        uint64_t before = 0, total = 0;
        for (int w = 0; w < kScanThreads / 64; ++w) {
            const uint64_t s = s_wave[w];
            if (w < wave) before += s;
            total += s;
        }
        uint64_t excl = carry + before + incl - sum;
#pragma unroll
        for (int q = 0; q < kScanPer; ++q) {
            const uint64_t l = e0 + q;
            const bool k = (keep >> q) & 1;
            if (l <= K) remap[l] = k ? (relabel ? (uint32_t)(excl + 1) : (uint32_t)l) : 0u;
            excl += k;
        }
        carry += total;
        __syncthreads();  // s_wave is written again in the next trip
    }
    if (largest) atomicMax(&s_largest, (ull)largest);
    __syncthreads();
    if (tid == 0) {
        kept[0] = carry;
        kept[1] = s_largest;
    }
}

// out[i] = remap[in[i]], 16 input bytes per lane and step where the input is 16-byte aligned.
template <int EI, int EO>
__global__ __launch_bounds__(kThreads) void lbl_gather_kernel(const uint8_t* __restrict__ in,
                                                              const uint32_t* __restrict__ remap,
                                                              uint8_t* __restrict__ out, int64_t n,
                                                              int aligned) {
    using UI = typename UIntOf<EI>::type;
    using UO = typename UIntOf<EO>::type;
    constexpr int PER = 16 / EI;
    const int64_t groups = (n + PER - 1) / PER;
    for (int64_t gidx = (int64_t)blockIdx.x * kThreads + threadIdx.x; gidx < groups;
         gidx += (int64_t)gridDim.x * kThreads) {
        const int64_t i0 = gidx * PER;
        UI e[PER];
        if (aligned && i0 + PER <= n) {
            const uint4 v = *reinterpret_cast<const uint4*>(in + i0 * EI);
            __builtin_memcpy(e, &v, 16);
        } else {
#pragma unroll
            for (int q = 0; q < PER; ++q)
                e[q] = i0 + q < n ? reinterpret_cast<const UI*>(in)[i0 + q] : (UI)0;
        }
#pragma unroll
        for (int q = 0; q < PER; ++q)
            if (i0 + q < n) reinterpret_cast<UO*>(out)[i0 + q] = (UO)remap[(uint64_t)e[q]];
    }
}

int env_int(const char* name, long lo, long hi, int dflt) {
    if (const char* e = std::getenv(name)) {
        const long v = std::atol(e);
        if (v >= lo && v <= hi) return (int)v;
    }
    return dflt;
}

template <int EL, int EI, bool COUNT>
hipError_t launch_stats_t(const void* lab, const void* inten, const LblGeom& g, const LblArgs& a,
                          int cols, void* state, hipStream_t s) {
    const int64_t cap = lbl_max_blocks();
    const unsigned grid = (unsigned)(g.tiles < cap ? g.tiles : cap);
    const size_t lds = (((size_t)a.slots * 4 + 7) & ~(size_t)7) + (size_t)cols * a.slots * 8;
    const int vec_l = ((uintptr_t)lab % 16 == 0) && ((uint64_t)g.X * EL) % 16 == 0;
    const int vec_i = EI && ((uintptr_t)inten % 16 == 0) && ((uint64_t)g.X * (EI ? EI : 1)) % 16 == 0;
    hipLaunchKernelGGL((lbl_stats_kernel<EL, EI, COUNT>), dim3(grid), dim3(kThreads), lds, s,
                       static_cast<const uint8_t*>(lab), static_cast<const uint8_t*>(inten), g, a,
                       vec_l, vec_i, static_cast<ull*>(state));
    return hipGetLastError();
}

template <int EL, bool COUNT>
hipError_t launch_stats_l(int esz_i, const void* lab, const void* inten, const LblGeom& g,
                          const LblArgs& a, int cols, void* state, hipStream_t s) {
    if constexpr (COUNT) {
        return launch_stats_t<EL, 0, true>(lab, nullptr, g, a, cols, state, s);
    } else {
        switch (esz_i) {
        case 0: return launch_stats_t<EL, 0, false>(lab, nullptr, g, a, cols, state, s);
        case 1: return launch_stats_t<EL, 1, false>(lab, inten, g, a, cols, state, s);
        case 2: return launch_stats_t<EL, 2, false>(lab, inten, g, a, cols, state, s);
        case 4: return launch_stats_t<EL, 4, false>(lab, inten, g, a, cols, state, s);
        case 8: return launch_stats_t<EL, 8, false>(lab, inten, g, a, cols, state, s);
        default: return hipErrorInvalidValue;
        }
    }
}

bool int_dtype(int d) { return d >= kI8 && d <= kU64; }

}  // namespace

int lbl_max_blocks() {
    // about 8 workgroups of 256 threads per CU, as info_max_blocks(); ZT_LABELS_MAX_BLOCKS lowers
    // it (tests reach the grid loop's second trip with a small array)
    return env_int("ZT_LABELS_MAX_BLOCKS", 1, 65535, 2048);
}

int lbl_slots(int cols) {
    // the LDS table's slots: a power of two, at most kLblSlots and kLblMaxTableBytes of LDS;
    // ZT_LABELS_LDS_SLOTS lowers it (tests reach probe collisions and the direct path)
    int want = env_int("ZT_LABELS_LDS_SLOTS", 1, kLblSlots, kLblSlots);
    int s = 1;
    while (s * 2 <= want) s *= 2;
    while (s > 1 && (size_t)s * (4 + 8 * (size_t)cols) > (size_t)kLblMaxTableBytes) s /= 2;
    return s;
}

bool lbl_intensity_sums(int dtype) {
    return dtype == kI8 || dtype == kI16 || dtype == kI32 || dtype == kU8 || dtype == kU16 ||
           dtype == kU32;
}

hipError_t launch_lbl_init(void* state, int ndim, int64_t n_labels, bool intensity,
                           bool count_only, hipStream_t s) {
    const int cols = lbl_cols(ndim, intensity, count_only);
    const uint64_t words = (uint64_t)cols * ((uint64_t)n_labels + 1) + 1;
    const uint64_t blocks = (words + kThreads - 1) / kThreads;
    const unsigned grid = (unsigned)(blocks < 2048 ? blocks : 2048);
    hipLaunchKernelGGL(lbl_init_kernel, dim3(grid), dim3(kThreads), 0, s, static_cast<ull*>(state),
                       (uint64_t)n_labels + 1, cols, ndim, count_only ? 1 : 0);
    return hipGetLastError();
}

hipError_t launch_lbl_accumulate(const void* labels, int dtype_labels, const void* intensity,
                                 int dtype_intensity, const int64_t* shape, const int64_t* origin,
                                 int ndim, int64_t n_labels, bool count_only, void* state,
                                 hipStream_t s) {
    if (!int_dtype(dtype_labels) || ndim < 1 || ndim > kMaxDims) return hipErrorInvalidValue;
    const bool with_i = intensity != nullptr && !count_only;
    if (with_i && (dtype_intensity < kI8 || dtype_intensity > kF64)) return hipErrorInvalidValue;
    LblGeom g;
    const int pad = kMaxDims - ndim;
    int64_t n = 1;
    for (int k = 0; k < kMaxDims; ++k) {
        g.dim[k] = k < pad ? 1 : shape[k - pad];
        g.org[k] = k < pad || !origin ? 0 : origin[k - pad];
        n *= g.dim[k];
    }
    if (n <= 0) return hipSuccess;
    g.X = g.dim[kMaxDims - 1];
    g.rows = n / g.X;
    g.segs = (g.X + 63) / 64;
    g.tiles = ((g.rows + T - 1) / T) * g.segs;
    g.ndim = ndim;
    LblArgs a;
    a.K = (uint64_t)n_labels;
    const int el = (int)dtype_size(dtype_labels);
    a.lab_neg = dtype_labels <= kI64 ? 1ull << (8 * el - 1) : 0;
    const int cols = lbl_cols(ndim, with_i, count_only);
    a.slots = lbl_slots(cols);
    a.i_sum = 0;
    a.i_fsign = a.i_pflip = a.i_nflip = a.i_sflip = 0;
    a.i_inf = ~0ull;
    int esz_i = 0;
    if (with_i) {
        esz_i = (int)dtype_size(dtype_intensity);
        const uint64_t sign = 1ull << (8 * esz_i - 1);
        a.i_sum = lbl_intensity_sums(dtype_intensity);
        if (dtype_intensity <= kI64) {
            a.i_pflip = a.i_nflip = a.i_sflip = sign;
        } else if (dtype_intensity >= kBF16) {
            a.i_fsign = a.i_pflip = sign;
            a.i_nflip = sign | (sign - 1);
            a.i_inf = dtype_intensity == kBF16 ? 0x7F80ull : dtype_intensity == kF16 ? 0x7C00ull
                      : dtype_intensity == kF32 ? 0x7F800000ull : 0x7FF0000000000000ull;
        }
    }
#define ZT_LBL_CASE(EL)                                                                          \
    case EL:                                                                                     \
        return count_only ? launch_stats_l<EL, true>(0, labels, nullptr, g, a, cols, state, s)   \
                          : launch_stats_l<EL, false>(esz_i, labels, intensity, g, a, cols,      \
                                                      state, s);
    switch (el) {
        ZT_LBL_CASE(1)
        ZT_LBL_CASE(2)
        ZT_LBL_CASE(4)
        ZT_LBL_CASE(8)
    default: return hipErrorInvalidValue;
    }
#undef ZT_LBL_CASE
}

hipError_t launch_lbl_keep_scan(const void* count_state, int64_t n_labels, uint64_t min_size,
                                uint64_t max_size, bool relabel, void* remap, void* kept,
                                hipStream_t s) {
    hipLaunchKernelGGL(lbl_keep_scan_kernel, dim3(1), dim3(kScanThreads), 0, s,
                       static_cast<const ull*>(count_state), (uint64_t)n_labels, min_size, max_size,
                       relabel ? 1 : 0, static_cast<uint32_t*>(remap), static_cast<uint64_t*>(kept));
    return hipGetLastError();
}

hipError_t launch_lbl_gather(const void* in, int dtype_in, const void* remap, void* out,
                             int dtype_out, int64_t n, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (!int_dtype(dtype_in) || !int_dtype(dtype_out)) return hipErrorInvalidValue;
    const int ei = (int)dtype_size(dtype_in), eo = (int)dtype_size(dtype_out);
    const int per = 16 / ei;
    const int64_t groups = (n + per - 1) / per, blocks = (groups + kThreads - 1) / kThreads;
    const int64_t cap = lbl_max_blocks();
    const unsigned grid = (unsigned)(blocks < cap ? blocks : cap);
    const int aligned = (uintptr_t)in % 16 == 0;
    const uint8_t* src = static_cast<const uint8_t*>(in);
    const uint32_t* map = static_cast<const uint32_t*>(remap);
    uint8_t* dst = static_cast<uint8_t*>(out);
#define ZT_LBL_GATHER(EI, EO)                                                                    \
    if (ei == EI && eo == EO) {                                                                  \
        hipLaunchKernelGGL((lbl_gather_kernel<EI, EO>), dim3(grid), dim3(kThreads), 0, s, src,   \
                           map, dst, n, aligned);                                                \
        return hipGetLastError();                                                                \
    }
    ZT_LBL_GATHER(1, 1) ZT_LBL_GATHER(1, 2) ZT_LBL_GATHER(1, 4) ZT_LBL_GATHER(1, 8)
    ZT_LBL_GATHER(2, 1) ZT_LBL_GATHER(2, 2) ZT_LBL_GATHER(2, 4) ZT_LBL_GATHER(2, 8)
    ZT_LBL_GATHER(4, 1) ZT_LBL_GATHER(4, 2) ZT_LBL_GATHER(4, 4) ZT_LBL_GATHER(4, 8)
    ZT_LBL_GATHER(8, 1) ZT_LBL_GATHER(8, 2) ZT_LBL_GATHER(8, 4) ZT_LBL_GATHER(8, 8)
#undef ZT_LBL_GATHER
    return hipErrorInvalidValue;
}

}  // namespace zt
