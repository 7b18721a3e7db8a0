// watershed.hip — the marker-controlled (seeded) watershed (an extension: the reference has no such
// filter).
//
// Every element of the domain D gets the label of one seed. Elements are compared only through the
// rank filters' order key (to_order_key; complemented when the relief is flooded from its
// maxima): the flood key. Four steps, each a pure function of the one before:
//
//   1. pass value c[p]: the least over paths in D from a seed of the greatest flood key on the
//      path. It is the reconstruction by erosion of J0 (the relief at seeds, the greatest key
//      elsewhere) under the relief: ws_init_kernel writes J0 (and the relief copy with the greatest
//      key outside D, when D is the foreground only) and reconstruct.hip's rounds do the rest.
//   2. plateau distance d[p] (uint32): 0 at seeds and where a D-neighbour has a smaller c, else
//      1 + the least d over D-neighbours of equal c. ws_dist_kernel, rounds of tiles like
//      reconstruct.hip's: a tile of d with a one-element apron in LDS, the equal-c neighbours of
//      every element as a bit set in registers, sweeps to a cap, the tile written to the other
//      buffer, one flag word per round.
//   3. parent: ws_parent_kernel, one pass: a seed is its own root; d = 0: the D-neighbour of least
//      (c, linear index) among those with smaller c; d > 0: the neighbour of least linear index
//      with equal c and d one less.
//   4. ws_jump_kernel: P' = P[P] between two buffers until a round changes nothing;
//      ws_gather_kernel: labels[p] = seeds[root(p)].
//
// In the d buffers kWsOut marks an element outside D (or outside the array, in an apron) and
// kWsNone one that no chain reaches yet; both are larger than any distance (n < 2^32 - 1). A round
// reads only what the launch before it finished writing. No kernel waits on another workgroup or
// spins on memory; every loop has a hard cap.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "zt_device.hpp"
#include "zt_gpu.hpp"
#include "zt_kernels.hpp"

namespace zt {

namespace {

constexpr int TZ = kRecTileZ, TY = kRecTileY, TX = kRecTileX;
constexpr int AZ = TZ + 2, AY = TY + 2, AX = TX + 2;  // the tile with its apron
constexpr int kThreads = TY * TX;                     // one thread per (y, x) column of the tile
constexpr int kFlatThreads = 256;
constexpr int kFlatMaxBlocks = 8192;  // the element-wise kernels are grid-strided beyond
static_assert(kThreads == 256, "four waves per workgroup");

constexpr uint32_t kWsNone = 0xFFFFFFFFu;  // no chain yet / no parent
constexpr uint32_t kWsOut = 0xFFFFFFFEu;   // outside D

// a seed element of `ssz` bytes at index i is a label when any bit is set
__device__ __forceinline__ bool ws_seeded(const uint8_t* seeds, int ssz, int64_t i) {
    switch (ssz) {
    case 1: return seeds[i] != 0;
    case 2: return reinterpret_cast<const uint16_t*>(seeds)[i] != 0;
    case 4: return reinterpret_cast<const uint32_t*>(seeds)[i] != 0;
    default: return reinterpret_cast<const uint64_t*>(seeds)[i] != 0;
    }
}

// ---- init ---------------------------------------------------------------------------------------

struct WsInit {
    const uint8_t* relief;
    const uint8_t* seeds;
    uint8_t* j0;
    uint8_t* domain;  // the relief with the greatest flood key outside D; null: D is everything
    uint32_t* d0;
    int64_t n;
    uint64_t fgmask;  // the storage bits that make a relief element foreground
    int32_t ssz, key_mode, descending;
    int32_t vec;  // relief, j0 and domain are 16-byte aligned
};

// 16 bytes of the relief per lane when its pointers are 16-byte aligned (the tail, fewer than
// 16 / ESZ elements, and every element otherwise go one by one). Every address comes from an index
// in [0, n).
template <int ESZ>
__global__ __launch_bounds__(kFlatThreads) void ws_init_kernel(const WsInit g) {
    using K = typename UIntOf<ESZ>::type;
    constexpr int V = 16 / ESZ;
    union Vec {
        uint4 q;
        K e[V];
    };
    const K* relief = reinterpret_cast<const K*>(g.relief);
    K* j0 = reinterpret_cast<K*>(g.j0);
    K* domain = reinterpret_cast<K*>(g.domain);
    const K comp = g.descending ? (K)~(K)0 : (K)0;
    const K top = from_order_key<K>((K)~(K)0, g.key_mode, comp);  // the greatest flood key, as bits
    const K m = (K)g.fgmask;
    const int64_t nvec = (g.n + V - 1) / V;
    for (int64_t v = (int64_t)blockIdx.x * kFlatThreads + threadIdx.x; v < nvec;
         v += (int64_t)gridDim.x * kFlatThreads) {
        const int64_t i0 = v * V;
        if (g.vec && i0 + V <= g.n) {
            Vec a, j, dm;
            a.q = *reinterpret_cast<const uint4*>(relief + i0);
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const bool in_d = !domain || (a.e[e] & m) != 0;
                const bool seeded = in_d && ws_seeded(g.seeds, g.ssz, i0 + e);
                j.e[e] = seeded ? a.e[e] : top;
                dm.e[e] = in_d ? a.e[e] : top;
                g.d0[i0 + e] = !in_d ? kWsOut : (seeded ? 0u : kWsNone);
            }
            *reinterpret_cast<uint4*>(j0 + i0) = j.q;
            if (domain) *reinterpret_cast<uint4*>(domain + i0) = dm.q;
        } else {
            for (int e = 0; e < V && i0 + e < g.n; ++e) {
                const K a = relief[i0 + e];
                const bool in_d = !domain || (a & m) != 0;
                const bool seeded = in_d && ws_seeded(g.seeds, g.ssz, i0 + e);
                j0[i0 + e] = seeded ? a : top;
                if (domain) domain[i0 + e] = in_d ? a : top;
                g.d0[i0 + e] = !in_d ? kWsOut : (seeded ? 0u : kWsNone);
            }
        }
    }
}

// ---- one round of the plateau distance ----------------------------------------------------------

struct WsDist {
    const uint8_t* c;     // pass values, storage bits
    const uint32_t* src;  // d of the round before
    uint32_t* dst;        // d of this round
    uint32_t* flag;       // this round's flag word: ORed with 1 when a tile changed
    const uint32_t* prev; // the flag word of the round before in this batch, or null
    int64_t Z, Y, X;      // the three innermost extents (front ones padded with 1)
    int64_t ty, tx;       // tiles along y and x
    int32_t connectivity; // 1 .. 3 on the three axes
    int32_t key_mode, descending, sweeps;
};

// bit of the neighbour at offset (dz, dy, dx) in an element's set of equal-c D-neighbours
__device__ __forceinline__ constexpr int ws_bit(int dz, int dy, int dx) {
    return (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1);
}

// the bits of the offsets that differ on 1 .. conn axes
__host__ __device__ constexpr uint32_t ws_allowed_bits(int conn) {
    uint32_t m = 0;
    for (int dz = -1; dz <= 1; ++dz)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                const int off = (dz != 0) + (dy != 0) + (dx != 0);
                if (off >= 1 && off <= conn) m |= 1u << ws_bit(dz, dy, dx);
            }
    return m;
}
__device__ __forceinline__ uint32_t ws_allowed(int conn) {
    constexpr uint32_t a1 = ws_allowed_bits(1), a2 = ws_allowed_bits(2), a3 = ws_allowed_bits(3);
    return conn <= 1 ? a1 : (conn == 2 ? a2 : a3);
}

// all ones unless bit `b` of `set` is set: ORed into a distance it makes "none"
__device__ __forceinline__ uint32_t ws_unless(uint32_t set, int b) {
    return ((set >> b) & 1u) - 1u;
}
// one more than a distance; "none" stays "none"
__device__ __forceinline__ uint32_t ws_next(uint32_t d) { return d == kWsNone ? kWsNone : d + 1; }

template <int ESZ>
__global__ __launch_bounds__(kThreads) void ws_dist_kernel(const WsDist g) {
    using K = typename UIntOf<ESZ>::type;
    // The round before changed nothing: both buffers already hold the fixed point. The word was
    // written by a launch that has finished; nothing here waits for anyone.
    if (g.prev && *g.prev == 0) return;
    __shared__ K sc[AZ * AY * AX];
    __shared__ uint32_t sd[AZ * AY * AX];
    const K comp = g.descending ? (K)~(K)0 : (K)0;
    const K* c = reinterpret_cast<const K*>(g.c);
    const int tid = threadIdx.x;
    const int64_t t = blockIdx.x;
    const int64_t z0 = (t / (g.ty * g.tx)) * TZ, y0 = ((t / g.tx) % g.ty) * TY,
                  x0 = (t % g.tx) * TX;
    // c keys and d of the tile and its apron; "outside D" outside the array
    for (int i = tid; i < AZ * AY * AX; i += kThreads) {
        const int ax = i % AX, ay = (i / AX) % AY, az = i / (AX * AY);
        const int64_t z = z0 + az - 1, y = y0 + ay - 1, x = x0 + ax - 1;
        K k = 0;
        uint32_t d = kWsOut;
        if (z >= 0 && z < g.Z && y >= 0 && y < g.Y && x >= 0 && x < g.X) {
            const int64_t q = (z * g.Y + y) * g.X + x;
            k = to_order_key<K>(c[q], g.key_mode, comp);
            d = g.src[q];
        }
        sc[i] = k;
        sd[i] = d;
    }
    __syncthreads();
    // this thread's column (ly, lx), z = 0 .. TZ - 1
    const int lx = tid % TX, ly = tid / TX;
    const int64_t gy = y0 + ly, gx = x0 + lx;
    const bool in_xy = gy < g.Y && gx < g.X;
    const int base = (ly + 1) * AX + (lx + 1);  // the column's (y, x) in a plane of the apron
    const int conn = g.connectivity;
    uint32_t cur[TZ], eq[TZ];
    // The equal-c D-neighbours of every element as a bit set, and d = 0 where a D-neighbour has a
    // smaller c: both depend on c alone, so every round finds them again. All 26 offsets are
    // looked at, column by column, and the ones the connectivity leaves out are masked off.
    bool changed = false;
    {
        const uint32_t allow = ws_allowed(conn);
        uint32_t lo[TZ];
        K cp[TZ];
#pragma unroll
        for (int z = 0; z < TZ; ++z) {
            cur[z] = sd[(z + 1) * AY * AX + base];
            cp[z] = sc[(z + 1) * AY * AX + base];
            eq[z] = 0;
            lo[z] = 0;
        }
        // one column per trip, not unrolled: the trips' loads and compares stay apart, which keeps
        // the registers low (the element itself sets its own bit; `allow` drops it)
#pragma unroll 1
        for (int k = 0; k < 9; ++k) {
            const int dy = k / 3 - 1, dx = k % 3 - 1;
            uint32_t dcol[AZ];
            K ccol[AZ];
#pragma unroll
            for (int z = 0; z < AZ; ++z) {
                dcol[z] = sd[z * AY * AX + base + dy * AX + dx];
                ccol[z] = sc[z * AY * AX + base + dy * AX + dx];
            }
#pragma unroll
            for (int z = 0; z < TZ; ++z) {
#pragma unroll
                for (int dz = -1; dz <= 1; ++dz) {
                    const uint32_t bit = 1u << ((dz + 1) * 9 + k);
                    const bool in_d = dcol[z + 1 + dz] != kWsOut;
                    eq[z] |= (in_d && ccol[z + 1 + dz] == cp[z]) ? bit : 0u;
                    lo[z] |= (in_d && ccol[z + 1 + dz] < cp[z]) ? bit : 0u;
                }
            }
        }
#pragma unroll
        for (int z = 0; z < TZ; ++z) {
            const bool lower = (lo[z] & allow) != 0 && cur[z] != kWsOut && cur[z] != 0;
            // outside D, a seed or a lower neighbour: fixed
            eq[z] = (cur[z] == kWsOut || cur[z] == 0 || lower) ? 0u : (eq[z] & allow);
            if (lower) {
                cur[z] = 0;
                changed = true;
            }
        }
    }
    __syncthreads();  // every read of the setup is done
    if (changed) {
#pragma unroll
        for (int z = 0; z < TZ; ++z) sd[(z + 1) * AY * AX + base] = cur[z];
    }
    bool tile_changed = __syncthreads_or(changed ? 1 : 0) != 0;
    for (int sweep = 0; sweep < g.sweeps; ++sweep) {
        // mn[z]: the least d over the equal-c neighbours; a neighbour whose bit is not set counts
        // as "none" (a set bit means an allowed neighbour in D, whose d is a distance or "none")
        uint32_t mn[TZ], nv[TZ];
#pragma unroll
        for (int z = 0; z < TZ; ++z) {
            mn[z] = kWsNone;
            // The 27 masks of an element do not change from sweep to sweep, and the compiler would
            // keep all 216 of a column in registers across the loop. An empty statement that
            // "writes" the set makes it derive them again: two cheap operations each.
            asm volatile("" : "+v"(eq[z]));
        }
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const int off = (dy != 0) + (dx != 0);  // axes this column differs on
                if (off > conn) continue;               // uniform over the workgroup
                uint32_t col[AZ];
#pragma unroll
                for (int z = 0; z < AZ; ++z) col[z] = sd[z * AY * AX + base + dy * AX + dx];
#pragma unroll
                for (int z = 0; z < TZ; ++z) {
#pragma unroll
                    for (int dz = -1; dz <= 1; ++dz) {
                        if (off + (dz != 0) == 0) continue;
                        mn[z] = kmin(mn[z], col[z + 1 + dz] | ws_unless(eq[z], ws_bit(dz, dy, dx)));
                    }
                }
            }
        }
#pragma unroll
        for (int z = 0; z < TZ; ++z) nv[z] = kmin(cur[z], ws_next(mn[z]));
        // along z inside the column: up, then down (each value stays a chain's length)
#pragma unroll
        for (int z = 1; z < TZ; ++z)
            nv[z] = kmin(nv[z], ws_next(nv[z - 1] | ws_unless(eq[z], ws_bit(-1, 0, 0))));
#pragma unroll
        for (int z = TZ - 2; z >= 0; --z)
            nv[z] = kmin(nv[z], ws_next(nv[z + 1] | ws_unless(eq[z], ws_bit(1, 0, 0))));
        changed = false;
#pragma unroll
        for (int z = 0; z < TZ; ++z) changed = changed || nv[z] != cur[z];
        __syncthreads();  // every read of this sweep is done
        if (changed) {
#pragma unroll
            for (int z = 0; z < TZ; ++z) {
                cur[z] = nv[z];
                sd[(z + 1) * AY * AX + base] = nv[z];
            }
        }
        if (!__syncthreads_or(changed ? 1 : 0)) break;
        tile_changed = true;
    }
    if (in_xy) {
#pragma unroll
        for (int z = 0; z < TZ; ++z)
            if (z0 + z < g.Z) g.dst[((z0 + z) * g.Y + gy) * g.X + gx] = cur[z];
    }
    if (tile_changed && tid == 0) atomicOr(g.flag, 1u);
}

// ---- parents ------------------------------------------------------------------------------------

struct WsParent {
    const uint8_t* c;
    const uint32_t* d;
    const uint8_t* seeds;
    uint32_t* parent;
    int64_t n, Z, Y, X;
    int32_t connectivity, key_mode, descending, ssz;
};

// One pass: the parent of every element as a linear index, or "none". Neighbours are visited in
// the order of their linear indices, so the first of equal rank is the one of least index.
template <int ESZ>
__global__ __launch_bounds__(kFlatThreads) void ws_parent_kernel(const WsParent g) {
    using K = typename UIntOf<ESZ>::type;
    const K* c = reinterpret_cast<const K*>(g.c);
    const K comp = g.descending ? (K)~(K)0 : (K)0;
    const int conn = g.connectivity;
    for (int64_t i = (int64_t)blockIdx.x * kFlatThreads + threadIdx.x; i < g.n;
         i += (int64_t)gridDim.x * kFlatThreads) {
        const uint32_t d = g.d[i];
        uint32_t parent = kWsNone;
        if (d < kWsOut) {
            if (ws_seeded(g.seeds, g.ssz, i)) {
                parent = (uint32_t)i;
            } else {
                const int64_t x = i % g.X, r = i / g.X, y = r % g.Y, z = r / g.Y;
                const K cp = to_order_key<K>(c[i], g.key_mode, comp);
                K best = cp;
#pragma unroll
                for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
                    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                        for (int dx = -1; dx <= 1; ++dx) {
                            const int off = (dz != 0) + (dy != 0) + (dx != 0);
                            if (off == 0 || off > conn) continue;
                            const int64_t qz = z + dz, qy = y + dy, qx = x + dx;
                            if (qz < 0 || qz >= g.Z || qy < 0 || qy >= g.Y || qx < 0 || qx >= g.X)
                                continue;
                            const int64_t q = (qz * g.Y + qy) * g.X + qx;
                            const uint32_t dq = g.d[q];
                            if (dq == kWsOut) continue;
                            const K cq = to_order_key<K>(c[q], g.key_mode, comp);
                            if (d == 0) {
                                if (cq < best) {
                                    best = cq;
                                    parent = (uint32_t)q;
                                }
                            } else if (parent == kWsNone && cq == cp && dq == d - 1) {
                                parent = (uint32_t)q;
                            }
                        }
            }
        }
        g.parent[i] = parent;
    }
}

// ---- pointer jumping and the labels -------------------------------------------------------------

// dst[i] = src[src[i]]. Every entry that is not "none" is an index in [0, n) whose own entry is
// not "none" (a parent is an element of the forest), so both loads are in bounds.
__global__ __launch_bounds__(kFlatThreads) void ws_jump_kernel(const uint32_t* src, uint32_t* dst,
                                                               int64_t n, uint32_t* flag,
                                                               const uint32_t* prev) {
    if (prev && *prev == 0) return;
    bool changed = false;
    for (int64_t i = (int64_t)blockIdx.x * kFlatThreads + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * kFlatThreads) {
        const uint32_t p = src[i];
        uint32_t pp = p;
        if (p != kWsNone && (int64_t)p < n) pp = src[p];
        changed = changed || pp != p;
        dst[i] = pp;
    }
    if (__syncthreads_or(changed ? 1 : 0) && threadIdx.x == 0) atomicOr(flag, 1u);
}

template <typename S>
__global__ __launch_bounds__(kFlatThreads) void ws_gather_kernel(const uint32_t* root,
                                                                 const S* seeds, S* labels,
                                                                 int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * kFlatThreads + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * kFlatThreads) {
        const uint32_t r = root[i];
        labels[i] = (r != kWsNone && (int64_t)r < n) ? seeds[r] : (S)0;
    }
}

unsigned flat_grid(int64_t items) {
    int64_t grid = (items + kFlatThreads - 1) / kFlatThreads;
    if (grid > kFlatMaxBlocks) grid = kFlatMaxBlocks;
    return (unsigned)(grid < 1 ? 1 : grid);
}

template <int ESZ>
hipError_t ws_init(const WsInit& g, hipStream_t s) {
    constexpr int V = 16 / ESZ;
    hipLaunchKernelGGL((ws_init_kernel<ESZ>), dim3(flat_grid((g.n + V - 1) / V)),
                       dim3(kFlatThreads), 0, s, g);
    return hipGetLastError();
}

template <int ESZ>
hipError_t ws_dist(const WsDist& g, int64_t tiles, hipStream_t s) {
    hipLaunchKernelGGL((ws_dist_kernel<ESZ>), dim3((unsigned)tiles), dim3(kThreads), 0, s, g);
    return hipGetLastError();
}

template <int ESZ>
hipError_t ws_parent(const WsParent& g, hipStream_t s) {
    hipLaunchKernelGGL((ws_parent_kernel<ESZ>), dim3(flat_grid(g.n)), dim3(kFlatThreads), 0, s, g);
    return hipGetLastError();
}

template <typename S>
hipError_t ws_gather(const uint32_t* root, const void* seeds, void* labels, int64_t n,
                     hipStream_t s) {
    hipLaunchKernelGGL((ws_gather_kernel<S>), dim3(flat_grid(n)), dim3(kFlatThreads), 0, s, root,
                       static_cast<const S*>(seeds), static_cast<S*>(labels), n);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_ws_init(const void* relief, int dtype, const void* seeds, int dtype_seeds,
                          void* j0, void* domain, uint32_t* d0, int64_t n, bool descending,
                          hipStream_t s) {
    WsInit g;
    g.relief = static_cast<const uint8_t*>(relief);
    g.seeds = static_cast<const uint8_t*>(seeds);
    g.j0 = static_cast<uint8_t*>(j0);
    g.domain = static_cast<uint8_t*>(domain);
    g.d0 = d0;
    g.n = n;
    g.fgmask = fg_mask(dtype);
    g.ssz = (int)dtype_size(dtype_seeds);
    g.key_mode = rank_key_mode(dtype);
    g.descending = descending ? 1 : 0;
    g.vec = (((uintptr_t)relief | (uintptr_t)j0 | (uintptr_t)domain) & 15) == 0;
    if (n <= 0) return hipSuccess;
    switch ((int)dtype_size(dtype)) {
    case 1: return ws_init<1>(g, s);
    case 2: return ws_init<2>(g, s);
    case 4: return ws_init<4>(g, s);
    case 8: return ws_init<8>(g, s);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_ws_dist_round(const void* c, int dtype, const uint32_t* src, uint32_t* dst,
                                const RecGeom& geom, int connectivity, bool descending, int sweeps,
                                uint32_t* flag, const uint32_t* prev, hipStream_t s) {
    WsDist g;
    g.c = static_cast<const uint8_t*>(c);
    g.src = src;
    g.dst = dst;
    g.flag = flag;
    g.prev = prev;
    g.Z = geom.Z; g.Y = geom.Y; g.X = geom.X;
    g.ty = (geom.Y + TY - 1) / TY;
    g.tx = (geom.X + TX - 1) / TX;
    g.connectivity = connectivity < 3 ? connectivity : 3;
    g.key_mode = rank_key_mode(dtype);
    g.descending = descending ? 1 : 0;
    g.sweeps = sweeps;
    const int64_t tiles = rec_tiles(geom);
    if (tiles <= 0) return hipSuccess;
    if (tiles > 0x7FFFFFFFll) return hipErrorInvalidValue;
    switch ((int)dtype_size(dtype)) {
    case 1: return ws_dist<1>(g, tiles, s);
    case 2: return ws_dist<2>(g, tiles, s);
    case 4: return ws_dist<4>(g, tiles, s);
    case 8: return ws_dist<8>(g, tiles, s);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_ws_parent(const void* c, int dtype, const uint32_t* d, const void* seeds,
                            int dtype_seeds, uint32_t* parent, const RecGeom& geom,
                            int connectivity, bool descending, hipStream_t s) {
    WsParent g;
    g.c = static_cast<const uint8_t*>(c);
    g.d = d;
    g.seeds = static_cast<const uint8_t*>(seeds);
    g.parent = parent;
    g.Z = geom.Z; g.Y = geom.Y; g.X = geom.X;
    g.n = geom.Z * geom.Y * geom.X;
    g.connectivity = connectivity < 3 ? connectivity : 3;
    g.key_mode = rank_key_mode(dtype);
    g.descending = descending ? 1 : 0;
    g.ssz = (int)dtype_size(dtype_seeds);
    if (g.n <= 0) return hipSuccess;
    switch ((int)dtype_size(dtype)) {
    case 1: return ws_parent<1>(g, s);
    case 2: return ws_parent<2>(g, s);
    case 4: return ws_parent<4>(g, s);
    case 8: return ws_parent<8>(g, s);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_ws_jump(const uint32_t* src, uint32_t* dst, int64_t n, uint32_t* flag,
                          const uint32_t* prev, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(ws_jump_kernel, dim3(flat_grid(n)), dim3(kFlatThreads), 0, s, src, dst, n,
                       flag, prev);
    return hipGetLastError();
}

hipError_t launch_ws_gather(const uint32_t* root, const void* seeds, int dtype_seeds, void* labels,
                            int64_t n, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    switch ((int)dtype_size(dtype_seeds)) {
    case 1: return ws_gather<uint8_t>(root, seeds, labels, n, s);
    case 2: return ws_gather<uint16_t>(root, seeds, labels, n, s);
    case 4: return ws_gather<uint32_t>(root, seeds, labels, n, s);
    case 8: return ws_gather<uint64_t>(root, seeds, labels, n, s);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace zt
