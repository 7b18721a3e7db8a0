// zt_kernels.hpp — kernel parameter blocks and launchers shared by the .hip translation units.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "gf_plan.hpp"

namespace zt {

constexpr int kMaxDims = 8;
constexpr int kMaxRadius = 127;         // reference: u8 radius, halo (radius*2) as u8 (guided_filter.rs:92)
constexpr int kFusedMaxRadius = 8;      // fused 2.5-D kernel instantiations
constexpr int kSepTreeMaxRadius = 16;   // separable path: tree sums up to here, sequential beyond

// Fused 3-D guided filter. Domain = the block windows clamp to ([0,nz) x [0,ny) x [0,nx)).
// Input element (z,y,x) lives at in + (z - in_z0)*in_sz + y*in_sy + x (x stride 1).
// Output element (z,y,x) of the region [oz0,oz0+onz) x [oy0,..) x [ox0,..) lives at
// out + (z-oz0)*out_sz + (y-oy0)*out_sy + (x-ox0).
struct GFParams {
    const void* in;
    void* out;
    int64_t in_sz, in_sy;
    int64_t out_sz, out_sy;
    int in_z0;
    int zlo, zhi;  // input planes present in `in`: [zlo, zhi) = [in_z0, in_z0 + rows) within [0, nz)
    int nz, ny, nx;
    int oz0, oy0, ox0;
    int onz, ony, onx;
    int zseg;  // output slices per workgroup march (normally the chunk depth)
    int tiles_x, tiles_y, nseg;
    int itx0, itx1, ity0, ity1;  // interior tile range (fused kernel, host-computed)
    float eps;
    float rcp_w3;  // RN(1 / (2r+1)^3): the interior window count's reciprocal (host-computed)
};

// N-d geometry for the separable path and downsample (C-order logical shapes).
struct NdGeom {
    int ndim;
    int64_t numel;
    int64_t shape[kMaxDims];
    int64_t in_strides[kMaxDims];
    int64_t out_start[kMaxDims];
    int64_t out_shape[kMaxDims];
    int64_t out_strides[kMaxDims];
    int64_t out_numel;
};

bool fused_supports_radius(int radius);
// element-type pairs with a direct fused instantiation; others are staged through f32
bool fused_direct_pair(int dtype_in, int dtype_out);
hipError_t launch_reencode_cast(const void* in, int dtype_in, void* out, int dtype_out, int64_t n,
                                hipStream_t s);
hipError_t launch_cast_to_f32_3d(const void* in, int dtype, int64_t sz, int64_t sy, float* out,
                                 int64_t nz, int64_t ny, int64_t nx, hipStream_t s);
hipError_t launch_cast_from_f32_3d(const float* in, int dtype, void* out, int64_t sz, int64_t sy,
                                   int64_t nz, int64_t ny, int64_t nx, hipStream_t s);
// pl = plan_fused (gf_plan.hpp) of p's geometry; it overrides p's zseg / tile / interior fields
hipError_t launch_guided_fused(const GFParams& p, const FusedPlan& pl, int dtype_in,
                               int dtype_out, int radius, hipStream_t stream);
// scratch must hold separable_scratch_floats(g.numel) floats: v | X (2n) | Y (2n), each region
// starting on a 16-byte boundary (the f64 / float2 views of X and Y stay aligned for odd n)
inline int64_t separable_pad(int64_t n) { return (n + 3) & ~(int64_t)3; }
inline int64_t separable_scratch_floats(int64_t n) { return 5 * separable_pad(n); }
hipError_t launch_guided_separable(const void* in, int dtype_in, void* out, int dtype_out,
                                   const NdGeom& g, int radius, float eps, float* scratch,
                                   hipStream_t s);

// 4-D guided filter (guided4d.hip): t-window sums of per-timepoint 3-D box sums, four kernels.
bool guided4d_supports(int radius);
int64_t guided4d_scratch_bytes(int64_t numel, bool gather);
// T <= 4 timepoints, r <= 2: both stages of every timepoint in one z-march (g4_fused.hip),
// f32 C-order input, no scratch.
bool guided4d_fused_supports(int radius, const NdGeom& g);
hipError_t launch_guided4d_fused(const float* v, void* out, int dtype_out, const NdGeom& g,
                                 int radius, float eps, hipStream_t s);
hipError_t launch_guided4d(const void* in, int dtype_in, void* out, int dtype_out,
                           const NdGeom& g, int radius, float eps, void* scratch, hipStream_t s);

// Downsample (downsample.rs:72-120). g.shape = input shape, g.out_shape = output shape,
// win = window per axis (min(stride, extent)).
struct DSParams {
    int ndim;
    int64_t in_shape[kMaxDims];
    int64_t out_shape[kMaxDims];
    int64_t win[kMaxDims];
    int64_t out_numel;
    int64_t win_numel;
};
hipError_t launch_downsample(const void* in, int dtype_in, void* out, int dtype_out,
                             const DSParams& p, bool discrete, hipStream_t s);
// nl (2 or 3) fused 2x2x2 mean (or mode: discrete) pyramid levels: shapes[0] = input,
// shapes[1..nl] = levels (each floor(previous / 2), every extent of shapes[0..nl-1] >= 2);
// outs[l-1] = level l.
bool pyramid_fused_dtype(int dtype, bool discrete);
// the fused pyramid grid (launch_pyramid_fused) for a level-1 shape fits the launch limits
bool pyramid_fused_grid_fits(const int64_t* level1_shape);
hipError_t launch_pyramid_fused(const void* in, int dtype, const int64_t (*shapes)[3], int nl,
                                void* const* outs, bool discrete, hipStream_t s);

// Gaussian pass along one axis (gaussian.hip): input region outer x n x inner (C order), output
// outer x on x inner with output k reading input positions around o0 + k (replicate edges).
constexpr int kGaussMaxTaps = 255;  // kernel_half_size <= 127 per axis
struct GaussPass {
    int64_t outer, n, on, o0, inner;
    int len, mid;
    float w[kGaussMaxTaps];
};
hipError_t launch_gaussian_pass(const void* in, int dtype_in, float* out, const GaussPass& p,
                                hipStream_t s);
// The last two axes' passes fused (y then x, tiles staged in LDS): input outer x ny x nx, output
// outer x py.on x px.on; py / px carry the two axes' taps, lengths, output offsets and extents.
constexpr int kGaussYXMaxLen = 33;
hipError_t launch_gaussian_yx(const void* in, int dtype_in, float* out, int64_t outer,
                              const GaussPass& py, const GaussPass& px, hipStream_t s);

// The last three axes' passes fused in one z-march (z, y then x; taps L on all three, odd,
// <= kGaussZYXMaxLen): input outer x nz x ny x nx, f32 output outer x on[0] x on[1] x on[2].
constexpr int kGaussZYXMaxLen = 13;
struct GaussZYX {
    int64_t outer, n[3], on[3], o0[3];
    int len;
    float w[3][kGaussZYXMaxLen];
};
bool gaussian_zyx_supported(const GaussZYX& p, int dtype_in);
hipError_t launch_gaussian_zyx(const void* in, int dtype_in, float* out, const GaussZYX& p,
                               hipStream_t s);

// Gradient magnitude (gradient.hip; gradient_magnitude.rs:109-147, kernel.rs:75-129).
// 3-D Sobel in one z-march: C-order input block n[3] of dtype_in, f32 output of the region
// [o0, o0 + on) (C order, on[3]); edges clamp at the block bounds.
constexpr int kGMSegMin = 32;  // fewest output slices per z segment
struct GMSobel3 {
    int64_t n[3], on[3], o0[3];
};
bool gm_sobel3_supported(const GMSobel3& p);
// output slices per z segment of the launch (and the segment count)
int gm_sobel3_zseg(const GMSobel3& p, int64_t* nseg);
hipError_t launch_gm_sobel3(const void* in, int dtype_in, float* out, const GMSobel3& p,
                            hipStream_t s);
// The generic passes on a whole C-order block: one triangle (diff = false) or difference pass
// along the axis of extent n (block = outer x n x inner, dtype_in -> f32); g = (first ? 0 : g) +
// s * s; out = sqrt(g) on the region g.out_start / g.out_shape of the block g.shape, as dtype_out.
hipError_t launch_gm_pass(const void* in, int dtype_in, float* out, int64_t outer, int64_t n,
                          int64_t inner, bool diff, hipStream_t s);
hipError_t launch_gm_accumulate(float* g, const float* sq, int64_t total, bool first,
                                hipStream_t s);
hipError_t launch_gm_finish(const float* g, int dtype_out, void* out, const NdGeom& geom,
                            hipStream_t s);

// Rank filters (rank.hip): minimum, median, maximum of the replicate-edge window
// of half sizes h. Elements are handled as their storage bits (esz = 1, 2, 4 or 8 bytes) under an
// order key chosen by `mode`; kind: kRank* (= ZT_RANK_*).
enum RankKind : int { kRankMinimum = 0, kRankMedian = 1, kRankMaximum = 2 };
enum RankKeyMode : int { kRankKeyUnsigned = 0, kRankKeySigned = 1, kRankKeyFloat = 2 };
constexpr int kRankSegMin = 32;           // fewest output slices per z segment (fused)
constexpr int64_t kRankMedianMaxWindow = 4096;
inline int rank_key_mode(int dtype) {
    switch (dtype) {
    case 1: case 2: case 3: case 4: return kRankKeySigned;     // kI8 .. kI64
    case 9: case 10: case 11: case 12: return kRankKeyFloat;   // kBF16, kF16, kF32, kF64
    default: return kRankKeyUnsigned;                          // kBool, kU8 .. kU64
    }
}
// 3-D, h = (1, 1, 1) in one z-march: C-order input block n[3], the region [o0, o0 + on) written
// C order (on[3]) in the input type; edges clamp at the block bounds.
struct Rank3 {
    int64_t n[3], on[3], o0[3];
};
bool rank3_supported(const Rank3& p, int esz);
int rank3_zseg(const Rank3& p, int64_t* nseg);
hipError_t launch_rank3(const void* in, void* out, int esz, int mode, int kind, const Rank3& p,
                        hipStream_t s);
// Minimum / maximum along one axis: input outer x n x inner (C order), output outer x on x inner,
// output k covering the input positions [o0 + k - h, o0 + k + h] clamped to the axis.
struct RankPass {
    int64_t outer, n, on, o0, h, inner;
};
hipError_t launch_rank_pass(const void* in, void* out, int esz, int mode, bool max,
                            const RankPass& p, hipStream_t s);
// Median by bisection: the region out_start / out_shape of the C-order block `shape` (C-order
// `stride`), window half sizes `half`; rows = prod(2 half[d] + 1) over every axis but the last,
// rank = (N - 1) / 2.
struct RankMedian {
    int ndim, rows, rank;
    int64_t out_numel;
    int64_t shape[kMaxDims], stride[kMaxDims], half[kMaxDims];
    int64_t out_start[kMaxDims], out_shape[kMaxDims];
};
hipError_t launch_rank_median(const void* in, void* out, int esz, int mode, const RankMedian& p,
                              hipStream_t s);

// Summed-area table (sat.hip; summed_area_table.rs:47-106): one inclusive running sum along the
// axis of extent n of a C-order array outer x n x inner, `element += acc` left to right in
// dtype_out, one thread per lane. in != out: the first pass (inner == 1 only), which casts
// dtype_in -> dtype_out on the way in; in == out (dtype_in == dtype_out): in place. seed / last:
// nullptr or outer * inner dtype_out values, the lanes' seeds (zero when null) and where their
// last values go; they may be the same buffer.
constexpr int kSatThreads = 256;  // threads per workgroup; lanes per workgroup when inner > 1
constexpr int kSatRows = 256;     // rows per workgroup of the x scan (inner == 1)
constexpr int kSatTileW = 32;     // x tile width of the x scan, output types of up to 4 bytes
constexpr int kSatTileW8 = 16;    // ... of 8 bytes
hipError_t launch_sat_pass(const void* in, int dtype_in, void* out, int dtype_out, int64_t outer,
                           int64_t n, int64_t inner, const void* seed, void* last, hipStream_t s);

// Pointwise programs (pointwise.hip; reencode.rs, crop.rs, rescale.rs, clamp.rs, equal.rs,
// replace_value.rs): 1..kPwMaxOps ops on every element of a box. Op k reads the type op k-1
// wrote (prog.dt_in for the first). Values are carried widened to a class (PwClass); the
// immediates are class values' bits: clamp a / b = min / max `as` the op's input type; equal and
// replace a = `value` in the input type; replace b = `replace` in the output type; rescale
// a / b = the f64 bits of multiply / add.
constexpr int kPwMaxOps = 8;
enum PwKind : int { kPwCast = 0, kPwRescale = 1, kPwClamp = 2, kPwEqual = 3, kPwReplace = 4 };
enum PwClass : int { kPwI32 = 0, kPwU32 = 1, kPwI64 = 2, kPwU64 = 3, kPwF32 = 4, kPwF64 = 5 };
constexpr int kPwAddFirst = 1;  // rescale: (x + add) * multiply
struct PwOp {
    int32_t kind, dt_out, flags, pad;
    uint64_t a, b;
};
struct PwProgram {
    int32_t n_ops, dt_in;
    PwOp ops[kPwMaxOps];
};
// The box as rows: `rows` rows of `row_len` contiguous source elements; row r starts at source
// element base + sum_d idx_d * stride[d], idx = r unravelled over shape[0..n_outer) (C order);
// the destination is contiguous. The launcher fills the fields below `stride`.
struct PwGeom {
    int64_t row_len, rows, base;
    int32_t n_outer;
    int64_t shape[kMaxDims - 1], stride[kMaxDims - 1];
    int32_t log2_g, rows32;
    int64_t segs, row_groups, step_rg, step_seg;
};
int pointwise_max_blocks();
hipError_t launch_pointwise(const void* in, void* out, PwGeom g, const PwProgram& prog,
                            hipStream_t s);

// Two-array arithmetic (arithmetic.hip; an extension, no reference filter): out[i] =
// (a[i] as f64 op b[i] as f64) as dt_out over n contiguous elements; the three pointers need
// element alignment only and `out` must not overlap a or b. A workgroup step is kArStepElems
// elements.
enum ArOp : int {
    kArAdd = 0, kArSubtract = 1, kArMultiply = 2, kArDivide = 3, kArMinimum = 4, kArMaximum = 5,
    kArAbsoluteDifference = 6, kArOps = 7
};
constexpr int kArThreads = 256;
constexpr int kArStepElems = 4096;
int arithmetic_max_blocks();
hipError_t launch_arithmetic(const void* a, int dt_a, const void* b, int dt_b, void* out,
                             int dt_out, int64_t n, int op, hipStream_t s);

// Connected-component labelling (connected.hip; an extension, no reference filter; DESIGN.md
// §3.13) of a contiguous C-order array of `shape` at element alignment. A workgroup of the local
// phase owns a tile of kCcTileZ x kCcTileY x kCcTileX elements of the three innermost axes
// (ZT_CC_TILE_* in the public header). Scratch (cc_scratch_bytes) holds two arrays of n indices
// (uint32_t, or uint64_t when cc_index64(n): n >= 2^32 - 1, or ZT_CC_INDEX64=1) and a tail: the
// component count K (kCcTailHeader bytes) and the host-built table of backward offsets, sized for
// the full neighbourhood of the rank. launch_cc_label runs everything up to the numbering and
// leaves K at cc_count_ptr; launch_cc_write then stores out[i] = label of i's component, or 0.
constexpr int kCcTileZ = 8, kCcTileY = 8, kCcTileX = 64;
constexpr int kCcBlockElems = 4096;  // elements of a numbering block
constexpr int kCcTailHeader = 64;
constexpr int64_t kCcMaxElems = (int64_t)1 << 38;
struct CcOffset {
    int64_t delta;  // linear index of the neighbour minus that of the element
    uint32_t d;     // offset + 1 on axis k of the shape padded in front to kMaxDims, 2 bits each
    uint32_t reserved;
};
bool cc_index64(int64_t n);
uint64_t cc_tail_bytes(int ndim);
uint64_t cc_scratch_bytes(int64_t n, bool idx64, int ndim);
const uint64_t* cc_count_ptr(const void* scratch, int64_t n, bool idx64);
hipError_t launch_cc_label(const void* in, int dtype_in, const int64_t* shape, int ndim,
                           int connectivity, bool idx64, void* scratch, hipStream_t s);
hipError_t launch_cc_write(const void* scratch, int64_t n, bool idx64, void* out, int dtype_out,
                           hipStream_t s);

// The exact Euclidean distance transform (distance.hip; an extension, no reference filter;
// DESIGN.md §3.14) of a contiguous C-order array of `shape` at element alignment: out = sqrt(d2)
// as dtype_out, or d2 itself with `squared`, d2 the squared distance to the nearest background
// (zero) element with `weight[a]` = spacing_a^2 per axis (zt_edt_host.hpp's edt_plan computes the
// weights, the bound B and whether it needs 64-bit work elements). Scratch (edt_scratch_bytes):
// two work arrays of n elements and the two stacks of n 4-byte slots. edt_work64 ORs the
// ZT_EDT_WORK64=1 switch into what B needs. Everything runs on `s`; nothing synchronises.
bool edt_work64(bool needed);
hipError_t launch_edt(const void* in, int dtype_in, const int64_t* shape, int ndim,
                      const uint64_t* weight, bool work64, void* scratch, void* out, int dtype_out,
                      int squared, hipStream_t s);

// Per-label statistics and the label size filter (labels.hip; extensions, no reference operation;
// DESIGN.md §3.15). The state's layout, size and limits are zt_labels_host.hpp's. A workgroup of
// the statistics owns tiles of kLblTileRows rows x 64 x of the box and an LDS table of at most
// kLblSlots labels (lbl_slots: fewer when the columns of a rank need it, or ZT_LABELS_LDS_SLOTS);
// the grid is capped at lbl_max_blocks() (ZT_LABELS_MAX_BLOCKS lowers it) and loops.
// launch_lbl_accumulate folds the contiguous C-order box `shape` at `origin` (NULL = zeros) of the
// whole array into `state`; intensity == NULL: no intensity columns; count_only: the count column
// alone. launch_lbl_keep_scan turns a count-only state into remap[0 .. K] (uint32_t: 0 for a label
// whose count is outside [min_size, max_size], else its rank among the kept ones + 1, or itself
// without `relabel`) and kept[0] = the kept count, kept[1] = the largest label kept;
// launch_lbl_gather writes out[i] = remap[in[i]] (every in[i] in [0, K]). Everything runs on `s`;
// nothing synchronises.
constexpr int kLblTileRows = 16;
constexpr int kLblSlots = 256;
int lbl_max_blocks();
int lbl_slots(int cols);
bool lbl_intensity_sums(int dtype);  // the six integer types of up to 32 bits
hipError_t launch_lbl_init(void* state, int ndim, int64_t n_labels, bool intensity,
                           bool count_only, hipStream_t s);
hipError_t launch_lbl_accumulate(const void* labels, int dtype_labels, const void* intensity,
                                 int dtype_intensity, const int64_t* shape, const int64_t* origin,
                                 int ndim, int64_t n_labels, bool count_only, void* state,
                                 hipStream_t s);
hipError_t launch_lbl_keep_scan(const void* count_state, int64_t n_labels, uint64_t min_size,
                                uint64_t max_size, bool relabel, void* remap, void* kept,
                                hipStream_t s);
hipError_t launch_lbl_gather(const void* in, int dtype_in, const void* remap, void* out,
                             int dtype_out, int64_t n, hipStream_t s);

// Morphological reconstruction (reconstruct.hip; an extension, no reference filter; DESIGN.md
// §3.16) of a contiguous C-order array at element alignment, seen as its three innermost axes
// (RecGeom: the axes in front of them all have extent 1). A workgroup of a round owns a tile of
// kRecTileZ x kRecTileY x kRecTileX elements (ZT_REC_TILE_* in the public header) and sweeps it at
// most rec_tile_sweeps() times (kRecTileSweeps: one crossing of the tile from corner to corner by
// faces; ZT_REC_TILE_SWEEPS=N, read at every call). The host launches rounds in batches of
// kRecBatch, each with its own flag word. Scratch (rec_scratch_bytes): one working array of the
// element type, padded to 16 bytes, and the flag words. launch_rec_init writes
// J0 = min(marker, mask) (max for erosion), or the generated marker of `marker_mode`, into `j0`;
// launch_rec_round writes one round of `src` into `dst`, ORs 1 into *flag when a tile changed, and
// does nothing when `prev` (the flag word of the round before, or NULL) is zero. Everything runs
// on `s`; nothing synchronises.
constexpr int kRecTileZ = 8, kRecTileY = 8, kRecTileX = 32;
constexpr int kRecTileSweeps = kRecTileZ + kRecTileY + kRecTileX;
constexpr int kRecBatch = 8;
constexpr int kRecTail = 64;  // the flag words of a batch
constexpr int64_t kRecMaxElems = (int64_t)1 << 38;
enum RecMarkerMode : int { kRecMarker = 0, kRecFillHoles = 1, kRecHMaxima = 2, kRecHMinima = 3 };
struct RecGeom {
    int64_t Z, Y, X;  // the three innermost extents, padded in front with 1
    int axes;         // how many of them are axes of the array: min(ndim, 3)
    bool unit_front;  // ndim > 3 (every axis in front of them has extent 1)
};
// false when an axis in front of the innermost three has an extent other than 1
inline bool rec_geom(const int64_t* shape, int ndim, RecGeom* g) {
    for (int d = 0; d + 3 < ndim; ++d)
        if (shape[d] != 1) return false;
    g->X = shape[ndim - 1];
    g->Y = ndim >= 2 ? shape[ndim - 2] : 1;
    g->Z = ndim >= 3 ? shape[ndim - 3] : 1;
    g->axes = ndim < 3 ? ndim : 3;
    g->unit_front = ndim > 3;
    return true;
}
inline int64_t rec_tiles(const RecGeom& g) {
    return ((g.Z + kRecTileZ - 1) / kRecTileZ) * ((g.Y + kRecTileY - 1) / kRecTileY) *
           ((g.X + kRecTileX - 1) / kRecTileX);
}
inline uint64_t rec_scratch_bytes(int64_t n, int esz) {
    return (((uint64_t)n * (uint64_t)esz + 15) & ~(uint64_t)15) + kRecTail;
}
inline uint32_t* rec_flags_ptr(void* scratch, int64_t n, int esz) {
    return reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(scratch) +
                                       (rec_scratch_bytes(n, esz) - kRecTail));
}
int rec_tile_sweeps();
hipError_t launch_rec_init(const void* mask, const void* marker, void* j0, int dtype,
                           const RecGeom& geom, int marker_mode, double h, bool erosion,
                           hipStream_t s);
hipError_t launch_rec_round(const void* src, const void* mask, void* dst, int dtype,
                            const RecGeom& geom, int connectivity, bool erosion, int sweeps,
                            uint32_t* flag, const uint32_t* prev, hipStream_t s);

// Seeded watershed (watershed.hip; an extension, no reference filter) of a
// contiguous C-order relief and a seeds array of an integer type, seen as reconstruction sees its
// arrays (RecGeom, the same tile, rec_tile_sweeps(), batches of kRecBatch). Scratch
// (ws_scratch_bytes), every part padded to 16 bytes: the two working arrays of the pass values
// (the relief's type), the relief with the greatest flood key outside the domain (the relief's
// type; only with `foreground_only`), two arrays of n uint32_t (the plateau distances, then the
// parents) and the flag words. launch_ws_init writes J0 into `j0`, the relief copy into `domain`
// (NULL: the domain is everything) and the first distances into `d0`; launch_ws_dist_round writes
// one round of `src` into `dst` from the pass values `c`, with the flag protocol of
// launch_rec_round; launch_ws_parent writes the parents from the final c and d; launch_ws_jump
// writes dst = src[src] and ORs 1 into *flag when an entry changed; launch_ws_gather writes
// labels[i] = seeds[root[i]], or 0. Everything runs on `s`; nothing synchronises.
constexpr int64_t kWsMaxElems = 0xFFFFFFFEll;  // n < 2^32 - 1: two index values are marks
inline uint64_t ws_pad16(uint64_t bytes) { return (bytes + 15) & ~(uint64_t)15; }
inline uint64_t ws_scratch_bytes(int64_t n, int esz, bool foreground_only) {
    return (foreground_only ? 3 : 2) * ws_pad16((uint64_t)n * (uint64_t)esz) +
           2 * ws_pad16((uint64_t)n * 4) + kRecTail;
}
// jump rounds of n elements: ceil(log2 n) + 2
inline int ws_jump_cap(int64_t n) {
    int bits = 0;
    while (((int64_t)1 << bits) < n) ++bits;
    return bits + 2;
}
hipError_t launch_ws_init(const void* relief, int dtype, const void* seeds, int dtype_seeds,
                          void* j0, void* domain, uint32_t* d0, int64_t n, bool descending,
                          hipStream_t s);
hipError_t launch_ws_dist_round(const void* c, int dtype, const uint32_t* src, uint32_t* dst,
                                const RecGeom& geom, int connectivity, bool descending, int sweeps,
                                uint32_t* flag, const uint32_t* prev, hipStream_t s);
hipError_t launch_ws_parent(const void* c, int dtype, const uint32_t* d, const void* seeds,
                            int dtype_seeds, uint32_t* parent, const RecGeom& geom,
                            int connectivity, bool descending, hipStream_t s);
hipError_t launch_ws_jump(const uint32_t* src, uint32_t* dst, int64_t n, uint32_t* flag,
                          const uint32_t* prev, hipStream_t s);
hipError_t launch_ws_gather(const uint32_t* root, const void* seeds, int dtype_seeds, void* labels,
                            int64_t n, hipStream_t s);

// zarrs_info reductions (info.hip; src/info/range.rs, src/info/histogram.rs) over a contiguous
// run of n elements of `dtype` (the 12 numeric types) at element alignment.
// Range: `state` is two device u64 words (smallest key, largest key) that accumulate across
// calls; launch_range_init makes them (all ones, 0) = "none". range_decode turns a key of the
// state back into the element's storage bits (zero-extended). NaN elements are ignored and
// -0.0 orders below +0.0.
// Histogram: adds into the device u64 hist[n_bins] the count of the elements of each bin,
// bin = min(floor(max((x as f64 - min) / (max - min) * n_bins, 0)) as usize, n_bins - 1)
// (histogram.rs:51-68). Up to kInfoLdsBins bins are privatised per workgroup in LDS.
constexpr int kInfoLdsBins = 4096;               // u32 LDS bins of a workgroup (16 KiB)
constexpr int64_t kInfoMaxBins = (int64_t)1 << 30;
int info_max_blocks();
hipError_t launch_range_init(void* state, hipStream_t s);
hipError_t launch_range_accumulate(const void* in, int dtype, int64_t n, void* state,
                                   hipStream_t s);
void range_decode(int dtype, uint64_t key, uint64_t* bits);
hipError_t launch_histogram_accumulate(const void* in, int dtype, int64_t n, int64_t n_bins,
                                       double mn, double mx, uint64_t* hist, hipStream_t s);

// zarrs_validate's per-element work (compare.hip; src/bin/zarrs_validate.rs:145-147): two
// contiguous runs a and b of n elements of `esz` bytes (1, 2, 4 or 8) at element alignment,
// compared by their storage bits. `state` is two device u64 words (differing elements, smallest
// differing index) that accumulate across calls; launch_compare_init makes them (0, all ones) =
// "equal". `base` is added to the run-local index.
hipError_t launch_compare_init(void* state, hipStream_t s);
hipError_t launch_compare_accumulate(const void* a, const void* b, int esz, int64_t n,
                                     int64_t base, void* state, hipStream_t s);

// Chunk occupancy (occupancy.hip; zarrs' `store_empty_chunks = false`, FillValue::equals_all): a
// contiguous C-order box of `shape` (ndim <= kMaxDims) elements of `esz` bytes (1, 2, 4 or 8) at
// element alignment, tiled from its origin by cells of `cell_shape` (the last cell of an axis may
// be partial). occupied[c] (device, one byte per cell, C order of the cell grid) becomes 1 when
// some element of cell c differs bitwise from the low `esz` bytes of fill_bits, else 0; the flags
// are cleared on `s` first. A box with a zero extent has no cells: nothing is launched.
hipError_t launch_chunk_occupancy(const void* data, int esz, const int64_t* shape, int ndim,
                                  const int64_t* cell_shape, uint64_t fill_bits, uint8_t* occupied,
                                  hipStream_t s);

// Synthetic inputs
hipError_t launch_synth_step_noise_f32(float* out, int64_t n, int64_t plane, int64_t nx_row,
                                       int64_t nx_global, int64_t z0, uint64_t seed,
                                       hipStream_t s);
hipError_t launch_synth_u16(uint16_t* out, int64_t n, int64_t plane, int64_t z0, uint64_t seed,
                            hipStream_t s);
hipError_t launch_synth_box(void* out, int kind, const int64_t* start, const int64_t* shape,
                            const int64_t* gshape, int ndim, uint64_t seed, hipStream_t s);

}  // namespace zt
