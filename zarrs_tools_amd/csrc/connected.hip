// connected.hip — connected-component labelling (an extension: the reference has no such filter;
// DESIGN.md §3.13) for gfx950.
//
// The working state is `parent`, one IdxT per element: a forest over the global C-order indices
// in which every edge points to a strictly smaller index (parent[x] <= x, equality at a root), so
// the root of a tree is the lowest index of its component, the component's first element.
//
//   cc_local_kernel        one workgroup per tile of kCcTileZ x kCcTileY x kCcTileX elements of
//                          the three innermost axes: loads the tile once, turns elements into
//                          foreground flags, labels the tile in LDS (x-runs by ballot, y / z and
//                          diagonal unions by union-find with LDS atomicMin, one compression pass)
//                          and writes parent[g] = global index of the local root (all ones for
//                          background)
//   cc_merge_faces_kernel  rank <= 3: the foreground elements on tile faces, united with their
//   cc_merge_all_kernel    backward neighbours in other tiles (global atomicMin); rank > 3: every
//                          element, since every offset on an outer axis leaves the tile
//   cc_flatten_count_kernel parent[i] = find(i), and the number of roots of each numbering block
//   cc_scan_kernel         one workgroup: exclusive prefix of the block counts, and K
//   cc_rank_kernel         label[root] = 1 + the number of roots before it in C order
//   cc_write_kernel        out[i] = foreground ? label[parent[i]] : 0
//
// Termination: find follows parent[] to strictly smaller indices until parent[a] == a; unite
// retries with a pair whose larger member is strictly smaller than before (see `unite`). No kernel
// waits for another workgroup, spins on a flag or depends on the order workgroups run in.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdlib>
#include <vector>

#include "zt_device.hpp"
#include "zt_gpu.hpp"
#include "zt_kernels.hpp"

namespace zt {

namespace {

constexpr int TZ = kCcTileZ, TY = kCcTileY, TX = kCcTileX;
constexpr int kRows = TZ * TY;          // x-rows of a tile
constexpr int kTileElems = kRows * TX;  // 4096
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kRowsPerWave = kRows / kWaves;
constexpr uint32_t kLdsBg = 0xFFFFFFFFu;
constexpr int kBlockIters = kCcBlockElems / kThreads;  // numbering: 64-element steps of a wave
static_assert(TX == 64, "a wave holds one x-row of a tile");
static_assert(kRows % kWaves == 0 && TY > 1 && TZ > 1, "tile shape");
static_assert(kCcBlockElems % kThreads == 0, "numbering block");


__device__ inline uint32_t amin(uint32_t* p, uint32_t v) { return atomicMin(p, v); }
__device__ inline uint64_t amin(uint64_t* p, uint64_t v) {
    return (uint64_t)atomicMin((unsigned long long*)p, (unsigned long long)v);
}

// The root of a's tree. Every step goes to a strictly smaller index (parent[x] < x for a
// non-root, whatever other threads store meanwhile: stores only lower an entry), so the loop ends
// after at most a steps.
template <typename T>
__device__ inline T find(const T* parent, T a) {
    for (T p = parent[a]; p != a; p = parent[a]) a = p;
    return a;
}

// Join the trees of a and b. With hi > lo two roots as this thread saw them, atomicMin(&parent[hi],
// lo) returns hi when hi still was a root: it now points to lo and the join is done. Otherwise
// another thread has given hi a parent `old` < hi in the meantime (and the atomicMin may have
// replaced it by lo): old's tree and lo's tree still have to be joined, so the loop goes on with
// (old, lo). Both are < hi, so the larger index of the pair strictly decreases from one trip to
// the next and the loop ends.
template <typename T>
__device__ inline void unite(T* parent, T a, T b) {
    for (;;) {
        a = find(parent, a);
        b = find(parent, b);
        if (a == b) return;
        if (a < b) {
            const T t = a;
            a = b;
            b = t;
        }
        const T old = amin(&parent[a], b);
        if (old == a) return;
        a = old;
    }
}

struct CcTiles {
    int64_t Z, Y, X;                   // the three innermost extents (unit axes for rank < 3)
    uint32_t tiles_z, tiles_y, tiles_x;  // tiles of one outer index
};

// ---- local phase -------------------------------------------------------------------------------

template <int ESZ, typename IdxT>
__global__ __launch_bounds__(kThreads) void cc_local_kernel(const uint8_t* __restrict__ in,
                                                            IdxT* __restrict__ parent, CcTiles g,
                                                            uint64_t fgmask, int conn, int vec_ok) {
    using U = typename UIntOf<ESZ>::type;
    __shared__ __attribute__((aligned(16))) uint8_t s_flag[kTileElems];
    __shared__ uint32_t s_lab[kTileElems];
    __shared__ uint64_t s_mask[kRows];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t b = blockIdx.x;
    const uint32_t tx = b % g.tiles_x;
    b /= g.tiles_x;
    const uint32_t ty = b % g.tiles_y;
    b /= g.tiles_y;
    const uint32_t tz = b % g.tiles_z;
    const int64_t outer = b / g.tiles_z;
    const int64_t z0 = (int64_t)tz * TZ, y0 = (int64_t)ty * TY, x0 = (int64_t)tx * TX;
    const int64_t obase = outer * g.Z * g.Y * g.X;
    const int nx = (int)(g.X - x0 < TX ? g.X - x0 : TX);
    const U m = (U)fgmask;

    // 1. the tile's elements, once, as foreground flags (one byte each)
    if (vec_ok && nx == TX) {
        constexpr int kPieces = 4 * ESZ;  // 16-byte pieces of a row
        constexpr int kRowsPerPass = kThreads / kPieces;
        constexpr int kPer = 16 / ESZ;    // elements of a piece
#pragma unroll
        for (int p = 0; p < kRows / kRowsPerPass; ++p) {
            const int row = p * kRowsPerPass + tid / kPieces, piece = tid % kPieces;
            const int64_t z = z0 + row / TY, y = y0 + row % TY;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (z < g.Z && y < g.Y)
                v = *reinterpret_cast<const uint4*>(
                    in + (uint64_t)(obase + (z * g.Y + y) * g.X + x0) * ESZ + piece * 16);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
            uint32_t f[4] = {0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < kPer; ++j) {
                U e;
                if constexpr (ESZ == 8) e = (U)w[2 * j] | ((U)w[2 * j + 1] << 32);
                else e = (U)(w[j * ESZ / 4] >> (8 * ((j * ESZ) % 4)));
                f[j / 4] |= (uint32_t)((e & m) != 0) << (8 * (j % 4));
            }
            uint8_t* dst = s_flag + row * TX + piece * kPer;
            if constexpr (kPer == 16) *reinterpret_cast<uint4*>(dst) = make_uint4(f[0], f[1], f[2], f[3]);
            else if constexpr (kPer == 8) *reinterpret_cast<uint2*>(dst) = make_uint2(f[0], f[1]);
            else if constexpr (kPer == 4) *reinterpret_cast<uint32_t*>(dst) = f[0];
            else *reinterpret_cast<uint16_t*>(dst) = (uint16_t)f[0];
        }
    } else {
        const U* src = reinterpret_cast<const U*>(in);
        for (int k = 0; k < kRowsPerWave; ++k) {
            const int row = wave * kRowsPerWave + k;
            const int64_t z = z0 + row / TY, y = y0 + row % TY;
            uint8_t f = 0;
            if (z < g.Z && y < g.Y && lane < nx)
                f = (src[obase + (z * g.Y + y) * g.X + x0 + lane] & m) != 0;
            s_flag[row * TX + lane] = f;
        }
    }
    __syncthreads();

    // 2. x-runs cost no union: a ballot of a row's flags gives every lane the start of its run
    for (int k = 0; k < kRowsPerWave; ++k) {
        const int row = wave * kRowsPerWave + k;
        const bool f = s_flag[row * TX + lane] != 0;
        const uint64_t mask = __ballot(f);
        if (lane == 0) s_mask[row] = mask;
        const uint64_t bg_below = ~mask & ((1ull << lane) - 1);
        const int start = bg_below ? 64 - __clzll((long long)bg_below) : 0;
        s_lab[row * TX + lane] = f ? (uint32_t)(row * TX + start) : kLdsBg;
    }
    __syncthreads();

    // 3. unions with the backward neighbours of the tile in the rows above (y - 1) and in the
    // plane before (z - 1). A, B: the flags of this row and of the neighbour row. Two elements
    // next to each other in A whose neighbours are next to each other in B need one union only
    // (the runs join the rest), and a diagonal neighbour (dx != 0) needs none when the straight
    // one (dx = 0) of this element or of the element beside it does the same job.
    for (int k = 0; k < kRowsPerWave; ++k) {
        const int row = wave * kRowsPerWave + k, lz = row / TY, ly = row % TY;
        const uint64_t A = s_mask[row];
        const uint32_t me = (uint32_t)(row * TX + lane);
#pragma unroll
        for (int dz = -1; dz <= 0; ++dz) {
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy) {
                if (dz == 0 && dy != -1) continue;  // not backward, or the x-run itself
                const int nnz = (dz != 0) + (dy != 0);
                const int nz_ = lz + dz, ny_ = ly + dy;
                if (nnz > conn || nz_ < 0 || ny_ < 0 || ny_ >= TY) continue;
                const int nrow = nz_ * TY + ny_;
                const uint64_t B = s_mask[nrow];
                const uint64_t C = A & B;
                if (((C & ~(C << 1)) >> lane) & 1) unite(s_lab, me, (uint32_t)(nrow * TX + lane));
                if (nnz + 1 <= conn) {
                    const uint64_t Um = A & (B << 1) & ~(A << 1) & ~B;
                    if ((Um >> lane) & 1) unite(s_lab, me, (uint32_t)(nrow * TX + lane - 1));
                    const uint64_t Up = A & (B >> 1) & ~(A >> 1) & ~B;
                    if ((Up >> lane) & 1) unite(s_lab, me, (uint32_t)(nrow * TX + lane + 1));
                }
            }
        }
    }
    __syncthreads();

    // 4. one compression pass; the local root is the lowest tile-local index of its local
    // component, and tile-local C order agrees with global C order inside a box
    const IdxT bg = ~(IdxT)0;
    for (int k = 0; k < kRowsPerWave; ++k) {
        const int row = wave * kRowsPerWave + k;
        const int64_t z = z0 + row / TY, y = y0 + row % TY;
        if (z >= g.Z || y >= g.Y || lane >= nx) continue;
        const uint32_t i = (uint32_t)(row * TX + lane);
        IdxT v = bg;
        if (s_lab[i] != kLdsBg) {
            const uint32_t r = find(s_lab, i);
            s_lab[i] = r;
            const int rrow = (int)(r / TX);
            v = (IdxT)(obase + ((z0 + rrow / TY) * g.Y + y0 + rrow % TY) * g.X + x0 + r % TX);
        }
        parent[obase + (z * g.Y + y) * g.X + x0 + lane] = v;
    }
}

// ---- merge phase -------------------------------------------------------------------------------

struct CcDims {
    int64_t dim[kMaxDims];  // the shape, padded in front with unit axes
};

// Unite element g (coordinates c) with its backward neighbours that lie in another tile.
template <int ND, typename IdxT>
__device__ inline void merge_element(IdxT* parent, int64_t g, const int64_t (&c)[kMaxDims],
                                     const CcDims& D, const CcOffset* __restrict__ offs, int noff) {
    const IdxT bg = ~(IdxT)0;
    if (parent[g] == bg) return;
    for (int j = 0; j < noff; ++j) {
        const int64_t delta = offs[j].delta;
        const uint32_t packed = offs[j].d;
        bool ok = true, cross = false;
#pragma unroll
        for (int k = kMaxDims - ND; k < kMaxDims; ++k) {
            const int d = (int)((packed >> (2 * k)) & 3u) - 1;
            const int64_t v = c[k] + d;
            ok = ok && v >= 0 && v < D.dim[k];
            if (k < kMaxDims - 3) cross = cross || d != 0;  // outer axes: tile extent 1
            else {
                const int sh = k == kMaxDims - 3 ? __builtin_ctz(TZ)
                               : k == kMaxDims - 2 ? __builtin_ctz(TY) : __builtin_ctz(TX);
                cross = cross || ((v >> sh) != (c[k] >> sh));
            }
        }
        if (!ok || !cross) continue;
        if (parent[g + delta] == bg) continue;
        unite(parent, (IdxT)g, (IdxT)(g + delta));
    }
}
static_assert((TZ & (TZ - 1)) == 0 && (TY & (TY - 1)) == 0 && (TX & (TX - 1)) == 0,
              "tile extents are powers of two");

// Rank <= 3. family: 0 = low z faces (z % TZ == 0, z > 0), 1 = low y, 2 = high y (y % TY == TY - 1,
// y < Y - 1), 3 = low x, 4 = high x; nk = faces of that family; total = threads. An element on
// faces of several families belongs to the first of them. High faces matter for diagonal offsets
// only (dy or dx = +1 behind a -1), so they are launched with connectivity >= 2 (hi != 0).
template <typename IdxT>
__global__ __launch_bounds__(kThreads) void cc_merge_faces_kernel(
    IdxT* parent, CcDims D, int family, int hi, int64_t nk, int64_t total,
    const CcOffset* __restrict__ offs, int noff) {
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= total) return;
    const int64_t Z = D.dim[kMaxDims - 3], Y = D.dim[kMaxDims - 2], X = D.dim[kMaxDims - 1];
    int64_t z, y, x;
    if (family == 0) {
        x = t % X;
        y = (t / X) % Y;
        z = (t / (X * Y) + 1) * TZ;
    } else if (family <= 2) {
        x = t % X;
        const int64_t k = (t / X) % nk;
        z = t / (X * nk);
        y = family == 1 ? (k + 1) * TY : k * TY + TY - 1;
    } else {
        const int64_t k = t % nk;
        y = (t / nk) % Y;
        z = t / (nk * Y);
        x = family == 3 ? (k + 1) * TX : k * TX + TX - 1;
    }
    const bool zlo = z > 0 && z % TZ == 0;
    const bool yface = (y > 0 && y % TY == 0) || (hi && y % TY == TY - 1 && y < Y - 1);
    if (family >= 1 && zlo) return;
    if (family >= 3 && yface) return;
    int64_t c[kMaxDims] = {0, 0, 0, 0, 0, z, y, x};
    merge_element<3, IdxT>(parent, (z * Y + y) * X + x, c, D, offs, noff);
}

// Rank > 3: every element.
template <typename IdxT>
__global__ __launch_bounds__(kThreads) void cc_merge_all_kernel(IdxT* parent, CcDims D, int64_t n,
                                                                const CcOffset* __restrict__ offs,
                                                                int noff) {
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= n) return;
    int64_t c[kMaxDims], r = t;
#pragma unroll
    for (int k = kMaxDims - 1; k >= 0; --k) {
        c[k] = r % D.dim[k];
        r /= D.dim[k];
    }
    merge_element<kMaxDims, IdxT>(parent, t, c, D, offs, noff);
}

// ---- flatten, number, write --------------------------------------------------------------------

// A numbering block is kCcBlockElems consecutive elements; wave w owns the w-th quarter and walks
// it in steps of 64, so a ballot and popcounts give the C-order rank of every root in the wave.
// The block's count, then its exclusive prefix, live in label[first element of the block], a slot
// that only this block ever writes.
template <typename IdxT>
__global__ __launch_bounds__(kThreads) void cc_flatten_count_kernel(IdxT* parent, IdxT* label,
                                                                    int64_t n) {
    __shared__ uint32_t s_cnt[kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const IdxT bg = ~(IdxT)0;
    const int64_t base = (int64_t)blockIdx.x * kCcBlockElems;
    const int64_t seg = base + (int64_t)wave * (kCcBlockElems / kWaves);
    uint32_t cnt = 0;
    for (int j = 0; j < kBlockIters; ++j) {
        const int64_t i = seg + j * 64 + lane;
        bool root = false;
        if (i < n) {
            const IdxT p = parent[i];
            if (p != bg) {
                const IdxT r = find(parent, p);
                if (r != p) parent[i] = r;
                root = r == (IdxT)i;
            }
        }
        cnt += (uint32_t)__popcll(__ballot(root));
    }
    if (lane == 0) s_cnt[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
        for (int w = 0; w < kWaves; ++w) s += s_cnt[w];
        label[base] = (IdxT)s;
    }
}

constexpr int kScanThreads = 1024, kScanPer = 8;

template <typename IdxT>
__global__ __launch_bounds__(kScanThreads) void cc_scan_kernel(IdxT* label, int64_t nb,
                                                               uint64_t* count) {
    __shared__ uint64_t s_wave[kScanThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint64_t carry = 0;
    for (int64_t c0 = 0; c0 < nb; c0 += kScanThreads * kScanPer) {
        const int64_t e0 = c0 + (int64_t)tid * kScanPer;
        uint64_t v[kScanPer], sum = 0;
#pragma unroll
        for (int q = 0; q < kScanPer; ++q) {
            v[q] = e0 + q < nb ? (uint64_t)label[(e0 + q) * kCcBlockElems] : 0;
            sum += v[q];
        }
        unsigned long long incl = sum;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned long long t = __shfl_up(incl, off, 64);
            if (lane >= off) incl += t;
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
            if (e0 + q < nb) label[(e0 + q) * kCcBlockElems] = (IdxT)excl;
            excl += v[q];
        }
        carry += total;
        __syncthreads();  // s_wave is written again in the next trip
    }
    if (tid == 0) *count = carry;
}

template <typename IdxT>
__global__ __launch_bounds__(kThreads) void cc_rank_kernel(const IdxT* __restrict__ parent,
                                                           IdxT* label, int64_t n) {
    __shared__ uint32_t s_cnt[kWaves];
    __shared__ uint64_t s_base;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t base = (int64_t)blockIdx.x * kCcBlockElems;
    const int64_t seg = base + (int64_t)wave * (kCcBlockElems / kWaves);
    // read before the barrier: element `base` may be a root, whose label lands in this slot
    if (threadIdx.x == 0) s_base = (uint64_t)label[base];
    uint64_t masks[kBlockIters];
    uint32_t cnt = 0;
#pragma unroll
    for (int j = 0; j < kBlockIters; ++j) {
        const int64_t i = seg + j * 64 + lane;
        masks[j] = __ballot(i < n && parent[i] == (IdxT)i);
        cnt += (uint32_t)__popcll(masks[j]);
    }
    if (lane == 0) s_cnt[wave] = cnt;
    __syncthreads();
    uint64_t rank = s_base;
    for (int w = 0; w < wave; ++w) rank += s_cnt[w];
#pragma unroll
    for (int j = 0; j < kBlockIters; ++j) {
        const uint64_t mk = masks[j];
        if ((mk >> lane) & 1)
            label[seg + j * 64 + lane] =
                (IdxT)(rank + (uint64_t)__popcll(mk & ((1ull << lane) - 1)) + 1);
        rank += (uint64_t)__popcll(mk);
    }
}

template <typename IdxT, typename TOut>
__global__ __launch_bounds__(kThreads) void cc_write_kernel(const IdxT* __restrict__ parent,
                                                            const IdxT* __restrict__ label,
                                                            TOut* __restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const IdxT p = parent[i];
    out[i] = p == ~(IdxT)0 ? (TOut)0 : (TOut)label[p];
}

// ---- host ----------------------------------------------------------------------------------------

// The backward half of the neighbourhood: offsets in {-1, 0, 1}^ndim whose first non-zero entry is
// -1, with at most `connectivity` non-zero entries, none on an axis of extent 1.
std::vector<CcOffset> backward_offsets(const int64_t* dim8, int ndim, int connectivity) {
    int64_t stride[kMaxDims];
    int64_t s = 1;
    for (int k = kMaxDims - 1; k >= 0; --k) {
        stride[k] = s;
        s *= dim8[k];
    }
    std::vector<CcOffset> out;
    int d[kMaxDims] = {0};
    const int first = kMaxDims - ndim;
    int64_t combos = 1;
    for (int k = 0; k < ndim; ++k) combos *= 3;
    for (int64_t code = 0; code < combos; ++code) {
        int64_t r = code;
        int nnz = 0, lead = 0;
        bool unit = false;
        for (int k = kMaxDims - 1; k >= first; --k) {
            d[k] = (int)(r % 3) - 1;
            r /= 3;
        }
        for (int k = first; k < kMaxDims; ++k) {
            if (d[k] == 0) continue;
            if (!lead) lead = d[k];
            ++nnz;
            unit = unit || dim8[k] == 1;
        }
        if (lead != -1 || nnz > connectivity || unit) continue;
        CcOffset o{0, 0, 0};
        for (int k = 0; k < kMaxDims; ++k) {
            const int dk = k >= first ? d[k] : 0;
            o.delta += dk * stride[k];
            o.d |= (uint32_t)(dk + 1) << (2 * k);
        }
        out.push_back(o);
    }
    return out;
}

template <typename IdxT>
hipError_t cc_label(const void* in, int dtype_in, const int64_t* shape, int ndim, int connectivity,
                    void* scratch, hipStream_t s) {
    CcDims D;
    for (int k = 0; k < kMaxDims; ++k)
        D.dim[k] = k < kMaxDims - ndim ? 1 : shape[k - (kMaxDims - ndim)];
    int64_t n = 1, outer = 1;
    for (int k = 0; k < kMaxDims; ++k) n *= D.dim[k];
    for (int k = 0; k < kMaxDims - 3; ++k) outer *= D.dim[k];
    const int64_t Z = D.dim[kMaxDims - 3], Y = D.dim[kMaxDims - 2], X = D.dim[kMaxDims - 1];
    if (n > kCcMaxElems) return hipErrorInvalidValue;  // so that no product below overflows
    const int64_t tiles_z = (Z + TZ - 1) / TZ, tiles_y = (Y + TY - 1) / TY,
                  tiles_x = (X + TX - 1) / TX;
    const int64_t tiles = outer * tiles_z * tiles_y * tiles_x;
    if (tiles > 0x7FFFFFFFll) return hipErrorInvalidValue;
    const CcTiles g{Z, Y, X, (uint32_t)tiles_z, (uint32_t)tiles_y, (uint32_t)tiles_x};

    IdxT* parent = static_cast<IdxT*>(scratch);
    IdxT* label = parent + n;
    uint8_t* tail = static_cast<uint8_t*>(scratch) + 2 * (size_t)n * sizeof(IdxT);
    uint64_t* count = reinterpret_cast<uint64_t*>(tail);
    CcOffset* offs = reinterpret_cast<CcOffset*>(tail + kCcTailHeader);

    const std::vector<CcOffset> table = backward_offsets(D.dim, ndim, connectivity);
    const int noff = (int)table.size();
    if (noff) {
        // pageable source: the copy has left `table` when the call returns
        hipError_t e = hipMemcpyAsync(offs, table.data(), sizeof(CcOffset) * table.size(),
                                      hipMemcpyHostToDevice, s);
        if (e != hipSuccess) return e;
    }

    const int esz = (int)dtype_size(dtype_in);
    const int vec_ok = ((uintptr_t)in % 16 == 0) && ((uint64_t)X * esz) % 16 == 0;
    const int conn3 = connectivity < 3 ? connectivity : 3;
    const uint64_t mask = fg_mask(dtype_in);
    const uint8_t* src = static_cast<const uint8_t*>(in);
    switch (esz) {
    case 1: cc_local_kernel<1, IdxT><<<(unsigned)tiles, kThreads, 0, s>>>(src, parent, g, mask, conn3, vec_ok); break;
    case 2: cc_local_kernel<2, IdxT><<<(unsigned)tiles, kThreads, 0, s>>>(src, parent, g, mask, conn3, vec_ok); break;
    case 4: cc_local_kernel<4, IdxT><<<(unsigned)tiles, kThreads, 0, s>>>(src, parent, g, mask, conn3, vec_ok); break;
    case 8: cc_local_kernel<8, IdxT><<<(unsigned)tiles, kThreads, 0, s>>>(src, parent, g, mask, conn3, vec_ok); break;
    default: return hipErrorInvalidValue;
    }
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;

    auto blocks = [](int64_t threads) { return (unsigned)((threads + kThreads - 1) / kThreads); };
    if (noff && ndim > 3 && outer > 1) {
        cc_merge_all_kernel<IdxT><<<blocks(n), kThreads, 0, s>>>(parent, D, n, offs, noff);
    } else if (noff) {
        const int hi = connectivity >= 2;
        const int64_t nk[5] = {(Z - 1) / TZ, (Y - 1) / TY, (Y - 1) / TY, (X - 1) / TX,
                               (X - 1) / TX};
        const int64_t per[5] = {Y * X, Z * X, Z * X, Z * Y, Z * Y};
        for (int f = 0; f < 5; ++f) {
            const int64_t total = nk[f] * per[f];
            if (total == 0 || ((f == 2 || f == 4) && !hi)) continue;
            cc_merge_faces_kernel<IdxT><<<blocks(total), kThreads, 0, s>>>(parent, D, f, hi, nk[f],
                                                                          total, offs, noff);
        }
    }
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;

    const int64_t nb = (n + kCcBlockElems - 1) / kCcBlockElems;
    cc_flatten_count_kernel<IdxT><<<(unsigned)nb, kThreads, 0, s>>>(parent, label, n);
    cc_scan_kernel<IdxT><<<1, kScanThreads, 0, s>>>(label, nb, count);
    cc_rank_kernel<IdxT><<<(unsigned)nb, kThreads, 0, s>>>(parent, label, n);
    return hipGetLastError();
}

template <typename IdxT>
hipError_t cc_write(const void* scratch, int64_t n, void* out, int dtype_out, hipStream_t s) {
    const IdxT* parent = static_cast<const IdxT*>(scratch);
    const IdxT* label = parent + n;
    const unsigned nb = (unsigned)((n + kThreads - 1) / kThreads);
    switch (dtype_size(dtype_out)) {  // a label fits the signed type too: the same bits
    case 1: cc_write_kernel<IdxT, uint8_t><<<nb, kThreads, 0, s>>>(parent, label, (uint8_t*)out, n); break;
    case 2: cc_write_kernel<IdxT, uint16_t><<<nb, kThreads, 0, s>>>(parent, label, (uint16_t*)out, n); break;
    case 4: cc_write_kernel<IdxT, uint32_t><<<nb, kThreads, 0, s>>>(parent, label, (uint32_t*)out, n); break;
    case 8: cc_write_kernel<IdxT, uint64_t><<<nb, kThreads, 0, s>>>(parent, label, (uint64_t*)out, n); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace

bool cc_index64(int64_t n) {
    // ZT_CC_INDEX64=1 forces the 64-bit instantiation (tests reach it with a small array)
    if (const char* e = std::getenv("ZT_CC_INDEX64"))
        if (e[0] == '1' && e[1] == 0) return true;
    return (uint64_t)n >= 0xFFFFFFFFull;
}

uint64_t cc_tail_bytes(int ndim) {
    uint64_t half = 1;
    for (int k = 0; k < ndim; ++k) half *= 3;
    return kCcTailHeader + sizeof(CcOffset) * ((half - 1) / 2);
}

uint64_t cc_scratch_bytes(int64_t n, bool idx64, int ndim) {
    return 2 * (uint64_t)n * (idx64 ? 8 : 4) + cc_tail_bytes(ndim);
}

const uint64_t* cc_count_ptr(const void* scratch, int64_t n, bool idx64) {
    return reinterpret_cast<const uint64_t*>(static_cast<const uint8_t*>(scratch) +
                                             2 * (size_t)n * (idx64 ? 8 : 4));
}

hipError_t launch_cc_label(const void* in, int dtype_in, const int64_t* shape, int ndim,
                           int connectivity, bool idx64, void* scratch, hipStream_t s) {
    return idx64 ? cc_label<uint64_t>(in, dtype_in, shape, ndim, connectivity, scratch, s)
                 : cc_label<uint32_t>(in, dtype_in, shape, ndim, connectivity, scratch, s);
}

hipError_t launch_cc_write(const void* scratch, int64_t n, bool idx64, void* out, int dtype_out,
                           hipStream_t s) {
    return idx64 ? cc_write<uint64_t>(scratch, n, out, dtype_out, s)
                 : cc_write<uint32_t>(scratch, n, out, dtype_out, s);
}

}  // namespace zt
