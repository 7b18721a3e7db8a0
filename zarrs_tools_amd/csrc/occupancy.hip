// occupancy.hip — which cells of a box hold anything but the fill value: what zarrs'
// `store_empty_chunks = false` asks of every chunk before it is stored (FillValue::equals_all),
// and the sharding codec of every inner chunk, answered for a whole output row while it still
// lies in device memory. The box is a contiguous C-order run of elements, the cells tile it from
// its origin (the last cell of an axis may be partial), and the answer is one byte per cell, in C
// order of the cell grid: 1 = some element's storage bits differ from the fill value's. The
// comparison is bitwise as in compare.hip: a NaN fill matches only its own payload, +0.0 is not
// -0.0, bool is a byte; the element's size is all that matters (1, 2, 4 and 8 bytes).
//
// The run is read as compare.hip reads one (zt_info.hpp): head, aligned 16-byte vectors, tail. A
// wave owns consecutive chunks of 64 x kOccUnroll vectors; a lane XORs its vectors with the fill
// pattern, and when a ballot finds no nonzero word in the wave (fill, the case that matters)
// nothing more happens. Otherwise the wave finds the row of the chunk's first element
// (zt_occupancy.hpp: the divisions, once per stretch of chunks with data; from chunk to chunk and
// row to row the position moves by additions and an odometer) and walks the rows that meet the
// chunk: a lane with a nonzero vector finds the cell of the vector's first element in the row (one
// division); a vector inside one cell marks it, one that straddles a cell or a row is attributed
// element by element. Flags only go from 0 to
// 1 with a plain byte store, so the result does not depend on the launch geometry. After a chunk
// with data the wave first looks at the flags of the next chunk's cells and does not load a chunk
// whose cells are all marked: dense data costs less than fill; the result never depends on it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "zt_info.hpp"
#include "zt_kernels.hpp"
#include "zt_occupancy.hpp"

namespace zt {

namespace {

constexpr int kOccUnroll = 4;                           // 16-byte vectors a lane loads per chunk
constexpr int64_t kOccChunkVecs = 64 * kOccUnroll;      // vectors of a wave's chunk (4 KiB)
constexpr int kOccWaves = kInfoThreads / 64;

template <int ESZ> struct OccUint;
template <> struct OccUint<1> { using type = uint8_t; };
template <> struct OccUint<2> { using type = uint16_t; };
template <> struct OccUint<4> { using type = uint32_t; };
template <> struct OccUint<8> { using type = uint64_t; };

// word w of a vector (selects: the vector stays in registers under a variable index)
__device__ __forceinline__ uint32_t word_of(const uint32_t (&x)[4], int w) {
    return w == 0 ? x[0] : w == 1 ? x[1] : w == 2 ? x[2] : x[3];
}

// element i of a vector's XOR with the fill pattern is nonzero
template <int ESZ>
__device__ __forceinline__ bool elem_differs(const uint32_t (&x)[4], int i) {
    if constexpr (ESZ == 8) return (word_of(x, 2 * i) | word_of(x, 2 * i + 1)) != 0;
    else if constexpr (ESZ == 4) return word_of(x, i) != 0;
    else if constexpr (ESZ == 2) return ((word_of(x, i >> 1) >> (16 * (i & 1))) & 0xFFFFu) != 0;
    else return ((word_of(x, i >> 2) >> (8 * (i & 3))) & 0xFFu) != 0;
}

template <int ESZ>
__global__ __launch_bounds__(kInfoThreads) void occupancy_kernel(
    const typename OccUint<ESZ>::type* p, const OccGeom g, int head, int64_t nvec,
    int64_t chunks_per_wave, uint32_t f0, uint32_t f1, typename OccUint<ESZ>::type fill,
    uint8_t* occ) {
    constexpr int PER = 16 / ESZ;
    const int lane = threadIdx.x & 63;
    const int64_t wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kOccWaves + (threadIdx.x >> 6)));
    const int64_t nchunks = (nvec + kOccChunkVecs - 1) / kOccChunkVecs;
    int64_t ch = wave * chunks_per_wave;
    const int64_t ch_end = ch + chunks_per_wave < nchunks ? ch + chunks_per_wave : nchunks;
    if (ch < ch_end) {
        const Vec16A* vp = reinterpret_cast<const Vec16A*>(p + head);
        OccRow st;           // where the chunk's first element lies, while `placed`
        bool placed = false;
        bool data = false;   // the wave's last chunk held something but fill
        for (; ch < ch_end; ++ch) {
            const int64_t vbase = ch * kOccChunkVecs;
            const int64_t nv = nvec - vbase < kOccChunkVecs ? nvec - vbase : kOccChunkVecs;
            const int64_t ne = nv * PER;
            if (data && placed && st.x + ne <= g.row) {  // in one row: are its cells marked?
                const int64_t k0 = st.x / g.cell_x, k1 = (st.x + ne - 1) / g.cell_x;
                if (k1 - k0 < 64) {
                    const bool open = lane <= k1 - k0 && occ[st.rowcell + k0 + lane] == 0;
                    if (__builtin_amdgcn_ballot_w64(open) == 0) {
                        st.advance(g, ne);
                        continue;
                    }
                }
            }
            uint32_t x[kOccUnroll][4], any = 0;
#pragma unroll
            for (int u = 0; u < kOccUnroll; ++u) {
                const int j = u * 64 + lane;
                Vec16A q;
                q.w[0] = q.w[2] = f0;  // a lane past the end: fill ^ fill
                q.w[1] = q.w[3] = f1;
                if (j < nv) q = vp[vbase + j];
                x[u][0] = q.w[0] ^ f0;
                x[u][1] = q.w[1] ^ f1;
                x[u][2] = q.w[2] ^ f0;
                x[u][3] = q.w[3] ^ f1;
                any |= x[u][0] | x[u][1] | x[u][2] | x[u][3];
            }
            if (__builtin_amdgcn_ballot_w64(any != 0) == 0) {  // the wave's vectors are fill
                data = false;
                // the position follows for free inside a row and is found again (init) if a
                // later chunk needs it: stretches of fill never step the odometer
                if (placed && st.x + ne < g.row) st.x += ne;
                else placed = false;
                continue;
            }
            data = true;
            if (!placed) {  // the divisions that find a row: once per stretch of data
                st.init(g, (int64_t)head + vbase * PER);
                placed = true;
            }
            // the rows that meet the chunk, [off, off + len) in the chunk's elements each
            int64_t off = 0;
            while (off < ne) {
                const int64_t len = ne - off < g.row - st.x ? ne - off : g.row - st.x;
#pragma unroll
                for (int u = 0; u < kOccUnroll; ++u) {
                    if ((x[u][0] | x[u][1] | x[u][2] | x[u][3]) == 0) continue;
                    const int64_t e0 = (int64_t)(u * 64 + lane) * PER;  // the vector's elements
                    const int64_t a = e0 > off ? e0 : off;
                    const int64_t b = e0 + PER < off + len ? e0 + PER : off + len;
                    if (a >= b) continue;
                    const int64_t xe = st.x + (a - off);
                    int64_t k = xe / g.cell_x, m = xe - k * g.cell_x;
                    if (m + (b - a) <= g.cell_x) {  // one cell holds all of them
                        bool some = b - a == PER;   // (the whole vector: it is nonzero)
#pragma unroll 1
                        for (int i = (int)(a - e0); !some && i < (int)(b - e0); ++i)
                            some = elem_differs<ESZ>(x[u], i);
                        if (some) occ[st.rowcell + k] = 1;
                        continue;
                    }
#pragma unroll 1
                    for (int i = (int)(a - e0); i < (int)(b - e0); ++i) {
                        if (elem_differs<ESZ>(x[u], i)) occ[st.rowcell + k] = 1;
                        if (++m == g.cell_x) {
                            m = 0;
                            ++k;
                        }
                    }
                }
                off += len;
                st.x += len;
                if (st.x == g.row) {
                    st.x = 0;
                    st.next_row(g);
                }
            }
        }
    }
    if (blockIdx.x == 0) {  // head and tail: fewer than one vector each
        const int64_t t0 = head + nvec * PER;
        if ((int)threadIdx.x < head && p[threadIdx.x] != fill)
            occ[occupancy_cell_of(g, threadIdx.x)] = 1;
        if (t0 + threadIdx.x < g.n && p[t0 + threadIdx.x] != fill)
            occ[occupancy_cell_of(g, t0 + threadIdx.x)] = 1;
    }
}

template <int ESZ>
hipError_t launch_occupancy_t(const void* data, const OccGeom& g, uint64_t fill_bits,
                              uint8_t* occ, hipStream_t s) {
    using U = typename OccUint<ESZ>::type;
    int head;
    int64_t nvec;
    static const int resident = resident_blocks(occupancy_kernel<ESZ>);  // asked once
    (void)split_run(resident, data, g.n, ESZ, &head, &nvec);
    int64_t cap = info_max_blocks();
    if (resident > 0 && resident < cap) cap = resident;
    const int64_t nchunks = (nvec + kOccChunkVecs - 1) / kOccChunkVecs;
    int64_t grid = (nchunks + kOccWaves - 1) / kOccWaves;
    grid = grid < 1 ? 1 : grid < cap ? grid : cap;
    const int64_t waves = grid * kOccWaves;
    const int64_t per_wave = (nchunks + waves - 1) / waves;
    uint64_t pat = fill_bits;  // the fill value repeated over 8 bytes
    if constexpr (ESZ < 8) pat &= ((uint64_t)1 << (8 * ESZ)) - 1;
    for (int b = ESZ; b < 8; b *= 2) pat |= pat << (8 * b);
    hipLaunchKernelGGL((occupancy_kernel<ESZ>), dim3((unsigned)grid), dim3(kInfoThreads), 0, s,
                       static_cast<const U*>(data), g, head, nvec, per_wave, (uint32_t)pat,
                       (uint32_t)(pat >> 32), (U)pat, occ);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_chunk_occupancy(const void* data, int esz, const int64_t* shape, int ndim,
                                  const int64_t* cell_shape, uint64_t fill_bits, uint8_t* occupied,
                                  hipStream_t s) {
    for (int d = 0; d < ndim; ++d)
        if (shape[d] <= 0) return hipSuccess;  // no element, no cell
    OccGeom g;
    occupancy_geom(shape, cell_shape, ndim, &g);
    hipError_t e = hipMemsetAsync(occupied, 0, (size_t)g.cells, s);
    if (e != hipSuccess) return e;
    switch (esz) {
    case 1: return launch_occupancy_t<1>(data, g, fill_bits, occupied, s);
    case 2: return launch_occupancy_t<2>(data, g, fill_bits, occupied, s);
    case 4: return launch_occupancy_t<4>(data, g, fill_bits, occupied, s);
    case 8: return launch_occupancy_t<8>(data, g, fill_bits, occupied, s);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace zt
