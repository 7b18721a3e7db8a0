// reconstruct.hip — morphological reconstruction of a marker under a mask (an extension: the
// reference has no such filter).
//
// By dilation: out is the least J >= J0 = min(marker, mask) with
//     J[p] = min(max(J[q] : q = p or a neighbour of p), mask[p])   for every p,
// neighbours as the labelling's (coordinates differ by at most 1 on every axis and on at most
// `connectivity` axes, nothing wraps). By erosion: the same with the order reversed. Elements are
// only ever selected under the rank filters' total order: storage bits become an unsigned key at
// every load (to_order_key; for erosion the key is complemented, which turns erosion into
// the dilation below) and a key becomes storage bits again at every store.
//
//   rec_init_kernel<ESZ>   J0 into the first working buffer: min(marker, mask), or a marker made
//                          from the mask (fill_holes, h_maxima, h_minima)
//   rec_round_kernel<ESZ>  one round: every workgroup owns a tile of kRecTileZ x Y x X elements of
//                          the three innermost axes, stages its J keys with a one-element apron in
//                          LDS (least key outside the array), holds its column's mask keys in
//                          registers, sweeps J <- min(max over the neighbourhood, mask) inside the
//                          tile with the apron fixed until a sweep changes nothing or the sweep
//                          cap is reached, writes the tile to the other working buffer and ORs
//                          into the round's flag word when anything in the tile changed
//
// A round reads only the buffer that the launch before it finished writing, so a round is a pure
// function of the one before: a sweep reads LDS, a barrier, then writes LDS, a barrier. No kernel
// waits on another workgroup or spins on memory; both loops have hard caps.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdlib>
#include <type_traits>

#include "zt_device.hpp"
#include "zt_gpu.hpp"
#include "zt_kernels.hpp"

namespace zt {

namespace {

constexpr int TZ = kRecTileZ, TY = kRecTileY, TX = kRecTileX;
constexpr int AZ = TZ + 2, AY = TY + 2, AX = TX + 2;  // the tile with its apron
constexpr int kThreads = TY * TX;                     // one thread per (y, x) column of the tile
constexpr int kInitThreads = 256;
static_assert(kThreads == 256, "four waves per workgroup");

// ---- the generated h marker: (mask as f64 -/+ h) as T, the arithmetic filter's casts ------------

template <typename T>
__device__ __forceinline__ uint64_t rec_shift_bits(uint64_t b, double h) {
    double x;
    if constexpr (std::is_same_v<T, bf16_t>) x = (double)bf16_bits_to_f32((uint16_t)b);
    else if constexpr (std::is_same_v<T, f16_t>) x = (double)f16_bits_to_f32((uint16_t)b);
    else if constexpr (std::is_same_v<T, float>) x = (double)u2f((uint32_t)b);
    else if constexpr (std::is_same_v<T, double>) x = __builtin_bit_cast(double, b);
    else x = (double)(T)b;  // i64 / u64: round to nearest even
    const T t = as_cast<double, T>(x + h);
    if constexpr (kIsHalf<T>) return t.bits;
    else if constexpr (std::is_same_v<T, float>) return f2u(t);
    else if constexpr (std::is_same_v<T, double>) return d2u(t);
    else return (uint64_t)(std::make_unsigned_t<T>)t;
}

template <int ESZ>
__device__ __forceinline__ uint64_t rec_shift(int dt, uint64_t b, double h) {
    if constexpr (ESZ == 1) {
        return dt == kI8 ? rec_shift_bits<int8_t>(b, h) : rec_shift_bits<uint8_t>(b, h);
    } else if constexpr (ESZ == 2) {
        return dt == kI16   ? rec_shift_bits<int16_t>(b, h)
               : dt == kF16 ? rec_shift_bits<f16_t>(b, h)
               : dt == kBF16 ? rec_shift_bits<bf16_t>(b, h)
                             : rec_shift_bits<uint16_t>(b, h);
    } else if constexpr (ESZ == 4) {
        return dt == kI32   ? rec_shift_bits<int32_t>(b, h)
               : dt == kF32 ? rec_shift_bits<float>(b, h)
                            : rec_shift_bits<uint32_t>(b, h);
    } else {
        return dt == kI64   ? rec_shift_bits<int64_t>(b, h)
               : dt == kF64 ? rec_shift_bits<double>(b, h)
                            : rec_shift_bits<uint64_t>(b, h);
    }
}

// ---- init ---------------------------------------------------------------------------------------

struct RecInit {
    const uint8_t* mask;
    const uint8_t* marker;  // kRecMarker only
    uint8_t* j0;
    int64_t n, Z, Y, X;  // elements; the three innermost extents (front ones padded with 1)
    double h;            // signed: -h for h_maxima, +h for h_minima
    int32_t marker_mode, dtype, key_mode, erosion;
    int32_t border_axes;  // fill_holes: how many of Z, Y, X are axes of the array (from the right)
    int32_t all_border;   // fill_holes: an axis in front of them has extent 1: every element is
    int32_t vec;          // every pointer is 16-byte aligned
};

template <int ESZ>
__device__ __forceinline__ typename UIntOf<ESZ>::type rec_init_one(
    const RecInit& g, int64_t i, typename UIntOf<ESZ>::type mask_bits,
    typename UIntOf<ESZ>::type marker_bits) {
    using K = typename UIntOf<ESZ>::type;
    const K comp = g.erosion ? (K)~(K)0 : (K)0;
    const K km = to_order_key<K>(mask_bits, g.key_mode, comp);
    K j;
    if (g.marker_mode == kRecMarker) {
        j = kmin(to_order_key<K>(marker_bits, g.key_mode, comp), km);
    } else if (g.marker_mode == kRecFillHoles) {
        bool border = g.all_border != 0;
        if (!border) {
            const int64_t x = i % g.X, r = i / g.X, y = r % g.Y, z = r / g.Y;
            border = x == 0 || x == g.X - 1;
            if (g.border_axes >= 2) border = border || y == 0 || y == g.Y - 1;
            if (g.border_axes >= 3) border = border || z == 0 || z == g.Z - 1;
        }
        j = border ? km : (K)0;  // the greatest key of the type, complemented
    } else {
        const K shifted = (K)rec_shift<ESZ>(g.dtype, (uint64_t)mask_bits, g.h);
        j = kmin(to_order_key<K>(shifted, g.key_mode, comp), km);
    }
    return from_order_key<K>(j, g.key_mode, comp);
}

// 16 bytes per lane when every pointer is 16-byte aligned (the tail, fewer than 16 / ESZ elements,
// and every element otherwise go one by one). Every address comes from an index in [0, n).
template <int ESZ>
__global__ __launch_bounds__(kInitThreads) void rec_init_kernel(const RecInit g) {
    using K = typename UIntOf<ESZ>::type;
    constexpr int V = 16 / ESZ;
    union Vec {
        uint4 q;
        K e[V];
    };
    const K* mask = reinterpret_cast<const K*>(g.mask);
    const K* marker = reinterpret_cast<const K*>(g.marker);
    K* j0 = reinterpret_cast<K*>(g.j0);
    const bool two = g.marker_mode == kRecMarker;
    const int64_t nvec = (g.n + V - 1) / V;
    for (int64_t v = (int64_t)blockIdx.x * kInitThreads + threadIdx.x; v < nvec;
         v += (int64_t)gridDim.x * kInitThreads) {
        const int64_t i0 = v * V;
        if (g.vec && i0 + V <= g.n) {
            Vec a, b, o;
            a.q = *reinterpret_cast<const uint4*>(mask + i0);
            b.q = two ? *reinterpret_cast<const uint4*>(marker + i0) : a.q;
#pragma unroll
            for (int e = 0; e < V; ++e) o.e[e] = rec_init_one<ESZ>(g, i0 + e, a.e[e], b.e[e]);
            *reinterpret_cast<uint4*>(j0 + i0) = o.q;
        } else {
            for (int e = 0; e < V && i0 + e < g.n; ++e) {
                const K a = mask[i0 + e];
                j0[i0 + e] = rec_init_one<ESZ>(g, i0 + e, a, two ? marker[i0 + e] : a);
            }
        }
    }
}

// ---- one round ----------------------------------------------------------------------------------

struct RecRound {
    const uint8_t* src;   // J of the round before
    const uint8_t* mask;
    uint8_t* dst;         // J of this round
    uint32_t* flag;       // this round's flag word: ORed with 1 when a tile changed
    const uint32_t* prev; // the flag word of the round before in this batch, or null
    int64_t Z, Y, X;      // the three innermost extents (front ones padded with 1)
    int64_t ty, tx;       // tiles along y and x
    int32_t connectivity; // 1 .. 3 on the three axes
    int32_t key_mode, erosion, sweeps;
};

template <int ESZ>
__global__ __launch_bounds__(kThreads) void rec_round_kernel(const RecRound g) {
    using K = typename UIntOf<ESZ>::type;
    // The round before changed nothing: both buffers already hold the fixed point. The word was
    // written by a launch that has finished; nothing here waits for anyone.
    if (g.prev && *g.prev == 0) return;
    __shared__ K sj[AZ * AY * AX];
    const K comp = g.erosion ? (K)~(K)0 : (K)0;
    const K* src = reinterpret_cast<const K*>(g.src);
    const K* mask = reinterpret_cast<const K*>(g.mask);
    K* dst = reinterpret_cast<K*>(g.dst);
    const int tid = threadIdx.x;
    const int64_t t = blockIdx.x;
    const int64_t z0 = (t / (g.ty * g.tx)) * TZ, y0 = ((t / g.tx) % g.ty) * TY,
                  x0 = (t % g.tx) * TX;
    // J keys of the tile and its apron; the least key outside the array
    for (int i = tid; i < AZ * AY * AX; i += kThreads) {
        const int ax = i % AX, ay = (i / AX) % AY, az = i / (AX * AY);
        const int64_t z = z0 + az - 1, y = y0 + ay - 1, x = x0 + ax - 1;
        K k = 0;
        if (z >= 0 && z < g.Z && y >= 0 && y < g.Y && x >= 0 && x < g.X)
            k = to_order_key<K>(src[(z * g.Y + y) * g.X + x], g.key_mode, comp);
        sj[i] = k;
    }
    // this thread's column (ly, lx), z = 0 .. TZ - 1: mask keys (the least key outside the array,
    // so that J stays the least key there)
    const int lx = tid % TX, ly = tid / TX;
    const int64_t gy = y0 + ly, gx = x0 + lx;
    const bool in_xy = gy < g.Y && gx < g.X;
    K m[TZ], cur[TZ];
#pragma unroll
    for (int z = 0; z < TZ; ++z) {
        m[z] = 0;
        if (in_xy && z0 + z < g.Z)
            m[z] = to_order_key<K>(mask[((z0 + z) * g.Y + gy) * g.X + gx], g.key_mode, comp);
    }
    __syncthreads();
    const int base = (ly + 1) * AX + (lx + 1);  // the column's (y, x) in a plane of sj
#pragma unroll
    for (int z = 0; z < TZ; ++z) cur[z] = sj[(z + 1) * AY * AX + base];
    const int conn = g.connectivity;
    bool tile_changed = false;
    for (int sweep = 0; sweep < g.sweeps; ++sweep) {
        K nv[TZ];
#pragma unroll
        for (int z = 0; z < TZ; ++z) nv[z] = cur[z];
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const int off = (dy != 0) + (dx != 0);  // axes this column differs on
                if (off > conn) continue;               // uniform over the workgroup
                K c[AZ];
#pragma unroll
                for (int z = 0; z < AZ; ++z) c[z] = sj[z * AY * AX + base + dy * AX + dx];
                if (off + 1 <= conn) {
#pragma unroll
                    for (int z = 0; z < TZ; ++z)
                        nv[z] = kmax(nv[z], kmax(kmax(c[z], c[z + 1]), c[z + 2]));
                } else {
#pragma unroll
                    for (int z = 0; z < TZ; ++z) nv[z] = kmax(nv[z], c[z + 1]);
                }
            }
        }
#pragma unroll
        for (int z = 0; z < TZ; ++z) nv[z] = kmin(nv[z], m[z]);
        // along z inside the column: up, then down (each value stays below the reconstruction)
#pragma unroll
        for (int z = 1; z < TZ; ++z) nv[z] = kmin(kmax(nv[z], nv[z - 1]), m[z]);
#pragma unroll
        for (int z = TZ - 2; z >= 0; --z) nv[z] = kmin(kmax(nv[z], nv[z + 1]), m[z]);
        bool changed = false;
#pragma unroll
        for (int z = 0; z < TZ; ++z) changed = changed || nv[z] != cur[z];
        __syncthreads();  // every read of this sweep is done
        if (changed) {
#pragma unroll
            for (int z = 0; z < TZ; ++z) {
                cur[z] = nv[z];
                sj[(z + 1) * AY * AX + base] = nv[z];
            }
        }
        if (!__syncthreads_or(changed ? 1 : 0)) break;
        tile_changed = true;
    }
    if (in_xy) {
#pragma unroll
        for (int z = 0; z < TZ; ++z)
            if (z0 + z < g.Z)
                dst[((z0 + z) * g.Y + gy) * g.X + gx] = from_order_key<K>(cur[z], g.key_mode, comp);
    }
    if (tile_changed && tid == 0) atomicOr(g.flag, 1u);
}

template <int ESZ>
hipError_t rec_init(const RecInit& g, hipStream_t s) {
    constexpr int V = 16 / ESZ;
    int64_t grid = ((g.n + V - 1) / V + kInitThreads - 1) / kInitThreads;
    if (grid > 8192) grid = 8192;  // grid-strided beyond
    hipLaunchKernelGGL((rec_init_kernel<ESZ>), dim3((unsigned)grid), dim3(kInitThreads), 0, s, g);
    return hipGetLastError();
}

template <int ESZ>
hipError_t rec_round(const RecRound& g, int64_t tiles, hipStream_t s) {
    hipLaunchKernelGGL((rec_round_kernel<ESZ>), dim3((unsigned)tiles), dim3(kThreads), 0, s, g);
    return hipGetLastError();
}

}  // namespace

int rec_tile_sweeps() {
    // ZT_REC_TILE_SWEEPS=N lowers or raises the in-tile cap (tests reach many rounds with 1)
    if (const char* e = std::getenv("ZT_REC_TILE_SWEEPS")) {
        const long v = std::atol(e);
        if (v >= 1 && v <= 65536) return (int)v;
    }
    return kRecTileSweeps;
}

hipError_t launch_rec_init(const void* mask, const void* marker, void* j0, int dtype,
                           const RecGeom& geom, int marker_mode, double h, bool erosion,
                           hipStream_t s) {
    RecInit g;
    g.mask = static_cast<const uint8_t*>(mask);
    g.marker = static_cast<const uint8_t*>(marker);
    g.j0 = static_cast<uint8_t*>(j0);
    g.n = geom.Z * geom.Y * geom.X;
    g.Z = geom.Z; g.Y = geom.Y; g.X = geom.X;
    g.h = marker_mode == kRecHMaxima ? -h : h;
    g.marker_mode = marker_mode;
    g.dtype = dtype;
    g.key_mode = rank_key_mode(dtype);
    g.erosion = erosion ? 1 : 0;
    g.border_axes = geom.axes;
    g.all_border = geom.unit_front ? 1 : 0;
    g.vec = (((uintptr_t)mask | (uintptr_t)j0 |
              (marker_mode == kRecMarker ? (uintptr_t)marker : (uintptr_t)0)) & 15) == 0;
    if (g.n <= 0) return hipSuccess;
    switch ((int)dtype_size(dtype)) {
    case 1: return rec_init<1>(g, s);
    case 2: return rec_init<2>(g, s);
    case 4: return rec_init<4>(g, s);
    case 8: return rec_init<8>(g, s);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_rec_round(const void* src, const void* mask, void* dst, int dtype,
                            const RecGeom& geom, int connectivity, bool erosion, int sweeps,
                            uint32_t* flag, const uint32_t* prev, hipStream_t s) {
    RecRound g;
    g.src = static_cast<const uint8_t*>(src);
    g.mask = static_cast<const uint8_t*>(mask);
    g.dst = static_cast<uint8_t*>(dst);
    g.flag = flag;
    g.prev = prev;
    g.Z = geom.Z; g.Y = geom.Y; g.X = geom.X;
    g.ty = (geom.Y + TY - 1) / TY;
    g.tx = (geom.X + TX - 1) / TX;
    g.connectivity = connectivity < 3 ? connectivity : 3;
    g.key_mode = rank_key_mode(dtype);
    g.erosion = erosion ? 1 : 0;
    g.sweeps = sweeps;
    const int64_t tiles = rec_tiles(geom);
    if (tiles <= 0) return hipSuccess;
    if (tiles > 0x7FFFFFFFll) return hipErrorInvalidValue;
    switch ((int)dtype_size(dtype)) {
    case 1: return rec_round<1>(g, tiles, s);
    case 2: return rec_round<2>(g, tiles, s);
    case 4: return rec_round<4>(g, tiles, s);
    case 8: return rec_round<8>(g, tiles, s);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace zt
